"""The block-packed symmetric GEMV (csrc/include/sym_gemv.h: part_block, reduce_row), the hot loop of
chain_big.hip, star_big.hip and first_order_big.hip, against the integer product -- bit for bit.

M is symmetric with integer entries uniform in [-2^19, 2^19], x likewise. Up to d = 8193 every partial sum
of every product stays below 8193 * 2^38 < 2^53, so every FMA and every addition is exact in ANY order and
``out[:d]`` must EQUAL the product formed in int64 (NumPy on the host; at d = 8193 torch on the device):
no tolerance. The kernel is called as ``ops.linalg.symv_packed`` calls it (``gadmm_symv_batch`` through
ctypes, ctl = None) on ``sym_pack`` of M. ``out`` and ``work`` are NaN before every call: ``out[:d]`` must
be finite and exact, ``out[d:]`` still NaN (only j < d is written), and a partial that reduce_row reads
and part_block never wrote surfaces as NaN.

tests/hp_reference.py has a NumPy model of the block structure; tests/test_hp_reference_cpu.py shows that
a dropped transposed product, a group clipped to its first eight partials and a direct product taken
with the wrong block of x each change the result on this data. profiles/star_classes/README.md records
the measured state of every shape.

Run with: pytest -m gpu tests/test_gpu_symv_exact.py -s
"""
import ctypes

import numpy as np
import pytest
import torch

import hp_reference as H

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
NAN = float("nan")

# d -> what it is the smallest d to reach (B = 128, nb = ceil(d / B), reduce_row: RG = 8 groups of
# per = ceil(nb / RG) partials, eight loads per trip)
SHAPES = [
    1,       # one block, one live element
    127,     # one diagonal block, padded
    128,     # one diagonal block, full
    129,     # nb = 2: the first transposed product; block row 1 has one live row
    255,     # nb = 2, padded
    256,     # nb = 2, full
    257,     # nb = 3
    1024,    # nb = 8 = RG: the last d with per = 1, every group holds one block
    1025,    # nb = 9: per = 2, the last group clipped at nb, groups 5..7 empty
    8193,    # nb = 65: per = 9, a second, masked trip of the eight-loads loop (the structure of d = 10 000)
]
assert tuple(SHAPES) == H.SYMV_SHAPES and max(SHAPES) == H.SYMV_MAX_D


@pytest.fixture(autouse=True)
def _poison_lds():
    """Every test starts with NaN-filled LDS on every CU (as tests/test_gpu.py)."""
    if torch.cuda.is_available():
        from gadmm_amd.ops import native
        native.poison_lds()
    yield


def _lib():
    from gadmm_amd.ops import native
    lib = native.require()
    fn = lib.gadmm_symv_batch
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long,
                   ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return native, fn


def _symv(Mp, mstride, xp, d, count):
    """``gadmm_symv_batch`` on ``count`` slots: ``Mp`` packed (stride ``mstride`` doubles), ``xp``
    (count, padded) zero padded. Returns out (count, padded), NaN wherever the kernel did not write."""
    from gadmm_amd.ops.linalg import sym_padded, symv_work_doubles
    native, fn = _lib()
    dp, wd = sym_padded(d), symv_work_doubles(d)
    nb = -(-d // H.SYMV_B)
    assert dp == nb * H.SYMV_B and wd == nb * nb * H.SYMV_B and xp.shape == (count, dp) and xp.is_contiguous()
    assert Mp.is_contiguous() and Mp.numel() >= (count - 1) * mstride + nb * (nb + 1) // 2 * H.SYMV_B ** 2
    out = torch.full((count, dp), NAN, dtype=torch.float64, device=DEV)
    work = torch.full((count * wd,), NAN, dtype=torch.float64, device=DEV)
    native.check(fn(Mp.data_ptr(), mstride, xp.data_ptr(), dp, out.data_ptr(), dp, work.data_ptr(), count, d, None,
                    native.stream_handle()), "symv_batch")
    torch.cuda.synchronize()
    return out


def _check(tag, out, want, d):
    """``out`` (count, padded) float64 against ``want`` (count, d) int64 (both on one device)."""
    head, tail = out[:, :d], out[:, d:]
    assert bool(torch.isfinite(head).all()), (tag, "NaN or inf in out[:d]: a partial nobody wrote")
    wrong = int((head != want.to(torch.float64)).sum())  # |want| < 2^53: the conversion is exact
    print("symv %s: %s (%d of %d entries differ), %d pad entries untouched"
          % (tag, "exact" if wrong == 0 else "NOT exact", wrong, head.numel(), tail.numel()))
    assert wrong == 0, (tag, wrong)
    assert bool(torch.isnan(tail).all()), (tag, "the kernel wrote past d")


def _host_case(d, count=1):
    from gadmm_amd.ops.linalg import sym_pack, sym_padded
    M, x, y = H.symv_int_data(d, count=count)
    Mf = torch.from_numpy(M.astype(np.float64)).to(DEV)
    xp = torch.zeros((count, sym_padded(d)), dtype=torch.float64, device=DEV)
    xp[:, :d] = torch.from_numpy(x.astype(np.float64)).to(DEV)
    return sym_pack(Mf), xp, torch.from_numpy(y).to(DEV)


def _device_case(d):
    """d = 8193: M, x and the int64 product are formed on the device (about 0.5 GB for M in int64, the same
    again in float64 and 0.3 GB packed; the int64 copies are gone before the kernel runs)."""
    from gadmm_amd.ops.linalg import sym_pack, sym_padded
    g = torch.Generator(device=DEV)
    g.manual_seed(7919 * d)
    A = torch.randint(-H.SYMV_AMP, H.SYMV_AMP + 1, (d, d), dtype=torch.int64, device=DEV, generator=g)
    M = torch.tril(A)
    M += torch.tril(A, -1).T
    del A
    x = torch.randint(-H.SYMV_AMP, H.SYMV_AMP + 1, (d,), dtype=torch.int64, device=DEV, generator=g)
    assert bool((M == M.T).all()) and int(M.abs().max()) <= H.SYMV_AMP
    y = torch.empty((d,), dtype=torch.int64, device=DEV)
    for r0 in range(0, d, 1024):  # row chunks: the elementwise product is the only temporary
        y[r0:r0 + 1024] = (M[r0:r0 + 1024] * x).sum(1)
    Mf = M.to(torch.float64)
    del M
    xp = torch.zeros((1, sym_padded(d)), dtype=torch.float64, device=DEV)
    xp[0, :d] = x.to(torch.float64)
    Mp = sym_pack(Mf.unsqueeze(0))
    del Mf
    return Mp, xp, y.unsqueeze(0)


@pytest.mark.parametrize("d", SHAPES)
def test_symv_packed_is_the_integer_product(d):
    Mp, xp, want = _host_case(d) if d < 8193 else _device_case(d)
    assert float(want.abs().max()) < 2.0 ** 53
    _check("d=%d" % d, _symv(Mp, Mp.shape[1], xp, d, 1), want, d)


def test_symv_batch_three_matrices():
    """count = 3 at d = 129: three matrices and three vectors, strides packed / padded / padded (the form
    of DGD, LAG and dual averaging in engine/first_order_big.py)."""
    d = 129
    Mp, xp, want = _host_case(d, count=3)
    assert Mp.shape[0] == 3 and not torch.equal(Mp[0], Mp[1]) and not torch.equal(want[0], want[2])
    _check("d=%d count=3" % d, _symv(Mp, Mp.shape[1], xp, d, 3), want, d)


def test_symv_batch_shared_matrix():
    """count = 2 at d = 257 with mstride = 0: one matrix, two vectors."""
    d = 257
    Mp, xp, want = _host_case(d, count=2)
    M, x, _ = H.symv_int_data(d, count=2)
    want = torch.from_numpy(np.stack([M[0].astype(np.int64) @ x[0], M[0].astype(np.int64) @ x[1]])).to(DEV)
    assert not torch.equal(want[0], want[1])
    _check("d=%d count=2 mstride=0" % d, _symv(Mp[0].contiguous(), 0, xp, d, 2), want, d)
