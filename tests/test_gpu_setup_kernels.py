"""The set-up kernels -- the three Grams and the SPD inverses -- against exact references.

The iterations consume what these kernels produce; the older tests hold them to torch float64 at fixed
normwise tolerances on well-conditioned Gaussian data, which one wrong small entry, a truncating slicer
or an unset status word all pass. Here:

(a) Integer-exact Gram. The data are integers times per-column powers of two with every partial sum
    below 2^53 (hp_reference.integer_gram_case), so the Gram is known EXACTLY: the f64-MFMA kernel
    (gram.hip, every split) and the digit kernel (gram_ozaki.hip: at most 3 non-zero digits per value,
    no digit pair dropped, every recombination step exact) must reproduce its float64 image bit for
    bit; the CRT kernel (gram_crt.hip) reconstructs the exact integer and evaluates it by Garner's
    Horner form, which rounds at most once per modulus above 2^53, so it stays within
    NMOD * 2^-53 * |exact| entrywise and gives exactly 0 where the exact entry is 0.
(b) The CRT kernel on full 49-bit images, against the Python-integer Gram, same entrywise bound.
(c) The three small inverse kernels (spd_inverse.hip) and (d) the blocked one (spd_inverse_blocked.hip)
    against the long-double inverse, on a well-conditioned family and on rank-deficient Grams plus a
    small shift (1e6 <= kappa <= 1e8). Per matrix

        max|out - ref| / max|ref| <= 8 * max(e64, d * 2^-53 * kappa)

    with e64 the error of the SAME recurrence in float64 NumPy (hp_reference.gauss_jordan_inverse).
(e) The non-SPD status word: set by a non-positive or NaN pivot at the first, a middle and the last
    index, raised as FloatingPointError, sticky, and not set by SPD input. A non-positive pivot is
    arithmetic (1 / p), not a device fault.

Every output tensor is pre-filled with NaN: an element a kernel does not write fails here instead of
inheriting an old value. Each test prints err / bound; profiles/setup_kernels/README.md records the
measured table. The CPU side of every reference is checked by tests/test_hp_reference_cpu.py.

Run with: pytest -m gpu tests/test_gpu_setup_kernels.py -s
"""
import numpy as np
import pytest
import torch

import hp_reference as H

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
NMOD = H.CRT_NMOD


@pytest.fixture(autouse=True)
def _poison_lds():
    """Every test starts with NaN-filled LDS on every CU (as tests/test_gpu.py)."""
    if torch.cuda.is_available():
        from gadmm_amd.ops import native
        native.poison_lds()
    yield


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)  # a copy: the cached references are read-only


def _host(t):
    return t.detach().cpu().numpy()


def _report(tag, ratios):
    """Print err / bound of every quantity, then assert all of them <= 1."""
    print("%s: err/bound %s" % (tag, " ".join("%s %.3g" % kv for kv in ratios.items())))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (tag, bad)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)


def _gram_out(g):
    n, d = g.N.shape[0], g.d
    return _nan(n, d, d), _nan(n, d), _nan(n)


def _written_and_symmetric(A, b, yy):
    A, b, yy = _host(A), _host(b), _host(yy)
    assert not (np.isnan(A).any() or np.isnan(b).any() or np.isnan(yy).any()), "an output element was not written"
    assert np.array_equal(A, A.transpose(0, 2, 1)), "A is not exactly symmetric"
    return A, b, yy


def _mismatch(g, A, b, yy):
    """Entries of (A, b, yy) that differ from the exact image, as err/bound figures: 0 passes."""
    return {"A": float(np.sum(A != g.A)), "b": float(np.sum(b != g.b)), "yy": float(np.sum(yy != g.yy))}


def _range_ratio(g, rng):
    ref = H.range_statistic(g)
    got = _host(rng).astype(H.LD)
    assert np.all(np.isfinite(_host(rng)))
    return float(np.max(np.abs(got - ref) / ref)) / (NMOD * 2.0 ** -53)


# ------------------------------------------------------------------------------------------------
# (a) integer-exact Gram
def _run_f64(g, ksplit):
    from gadmm_amd.ops import linalg
    out = _gram_out(g)
    res = linalg.gram(_dev(g.X), _dev(g.y), ksplit=ksplit, out=out)
    assert all(r.data_ptr() == o.data_ptr() for r, o in zip(res, out))
    A, b, yy = _written_and_symmetric(*out)
    assert torch.equal(out[0].cpu(), torch.from_numpy(np.array(g.A))) and torch.equal(out[1].cpu(), torch.from_numpy(
        np.array(g.b))) and torch.equal(out[2].cpu(), torch.from_numpy(np.array(g.yy))), _mismatch(g, A, b, yy)
    return _mismatch(g, A, b, yy)


# gadmm_gram_f64: BT = 64 while d + 1 <= 64 (d = 1, 62, 63), else 128 (64: the first; 126, 127: one
# tile, the y column its last / the first of a second tile; 128, 129, 255: 2 x 2 tiles, the last
# almost empty / full). BK = 16: m = 1, 15 (one partial slab), 16 (one full), 17, 33 (full + partial).
@pytest.mark.parametrize("d", H.GRAM_F64_D)
@pytest.mark.parametrize("m", H.GRAM_F64_M)
def test_gram_f64_integer_exact(m, d):
    _report("gram f64 (m %d, d %d) mismatches" % (m, d), _run_f64(H.gram_int_case(m, d), 1))


# launch_gram rounds the rows per split up to BK and recomputes the split count: (40, 3) -> 16, 16, 8;
# (33, 4) -> THREE splits of 16, 16, 1; (512, 2) -> 256, 256; (513, 2) -> 272, 241. Both tile sizes.
@pytest.mark.parametrize("d", H.GRAM_F64_SPLIT_D)
@pytest.mark.parametrize("m,ksplit", H.GRAM_F64_SPLIT)
def test_gram_f64_split_k_integer_exact(m, ksplit, d):
    _report("gram f64 split-K (m %d, d %d, ksplit %d) mismatches" % (m, d, ksplit),
            _run_f64(H.gram_int_case(m, d), ksplit))


def test_gram_f64_auto_split_integer_exact():
    """``ksplit=None``: the heuristic's own choice (gadmm_gram_pick_ksplit) at 2 x 1025 x 70."""
    from gadmm_amd.ops import linalg, native
    n, m, d = H.GRAM_F64_AUTO
    k = int(native.require().gadmm_gram_pick_ksplit(n, m, d))
    assert not linalg.gram_uses_ozaki(m, d)
    _report("gram f64 auto split (m %d, d %d, picked %d) mismatches" % (m, d, k), _run_f64(H.gram_int_case(m, d), None))


def _run_digits(g):
    from gadmm_amd.ops import linalg
    out = _gram_out(g)
    A_, b_, yy_, rng = linalg.gram_ozaki(_dev(g.X), _dev(g.y), out=out, with_range=True)
    A, b, yy = _written_and_symmetric(*out)
    r = _mismatch(g, A, b, yy)
    r["range"] = _range_ratio(g, rng)
    assert torch.equal(A_.cpu(), torch.from_numpy(np.array(g.A))) and torch.equal(b_.cpu(), torch.from_numpy(
        np.array(g.b))) and torch.equal(yy_.cpu(), torch.from_numpy(np.array(g.yy))), r
    return r


# gram_ozaki.hip: tile 64 (d + 1 = 2; 63; 64: one tile exactly full; 65: a second tile with one
# column; 130: a third), 32-sample blocks (m = 1, 31, 32, 33).
@pytest.mark.parametrize("d", H.GRAM_OZ_D)
@pytest.mark.parametrize("m", H.GRAM_OZ_M)
def test_gram_digits_integer_exact(m, d):
    _report("gram digits (m %d, d %d) mismatches" % (m, d), _run_digits(H.gram_int_case(m, d)))


# chunks of 8192 samples: one short of a chunk, exactly one, one sample into the second, one into the
# third (the slicer waits for the GEMM of the same digit buffer); two shards reuse both buffers.
@pytest.mark.parametrize("m", H.GRAM_OZ_LONG)
def test_gram_digits_chunk_edges_integer_exact(m):
    _report("gram digits (m %d, d 3) mismatches" % m, _run_digits(H.gram_int_case(m, 3)))


def _crt_ratios(g, out, rng=None):
    A, b, yy = _written_and_symmetric(*out)
    worst, nz = H.gram_errors(g, A, b, yy, lower_only=True)
    r = {"entry": worst / NMOD, "nonzero-at-exact-0": float(nz)}
    if rng is not None:
        r["range"] = _range_ratio(g, rng)
    return r


def _run_crt(g):
    from gadmm_amd.ops import linalg
    out = _gram_out(g)
    rng = linalg.gram_crt(_dev(g.X), _dev(g.y), out=out, with_range=True)[3]
    r = _crt_ratios(g, out, rng)
    assert r["nonzero-at-exact-0"] == 0.0, r
    return r


# gram_crt.hip: tile 256 (d + 1 = 2; 255; 256: one tile exactly full; 257: a second tile with one
# column), stages of 64 samples through a ring of 4 with a two-deep fragment pipeline: 1 .. 6 stages,
# each with a full and a one-sample-over tail.
@pytest.mark.parametrize("d", H.GRAM_CRT_D)
@pytest.mark.parametrize("m", H.GRAM_CRT_M)
def test_gram_crt_integer_family(m, d):
    _report("gram crt (m %d, d %d)" % (m, d), _run_crt(H.gram_int_case(m, d)))


# chunks of 32768 samples: exactly one, one sample into the second, one into the third (the slicer
# waits for the previous GEMM of the same residue buffer; the epilogue's first = 0 path).
@pytest.mark.parametrize("m", H.GRAM_CRT_LONG)
def test_gram_crt_chunk_edges_integer_family(m):
    _report("gram crt (m %d, d 3)" % m, _run_crt(H.gram_int_case(m, 3)))


# (b) the kernel counterpart of tests/test_gram_crt_math.py::test_emulated_gram_is_exact
@pytest.mark.parametrize("m,d", H.GRAM_IMAGE)
def test_gram_crt_full_49_bit_images(m, d):
    from gadmm_amd.ops import linalg
    g = H.image_case(2, m, d)
    out = _gram_out(g)
    linalg.gram_crt(_dev(g.X), _dev(g.y), out=out)
    _report("gram crt 49-bit images (m %d, d %d)" % (m, d), _crt_ratios(g, out))


# ------------------------------------------------------------------------------------------------
# (c) small inverses. gadmm_spd_inverse_small_f64 reads its switches per call.
SMALL_KERNELS = {"register": {}, "lds64": {"GADMM_INV_REG": "0"}, "general": {"GADMM_GJ64": "0"}}


def _small_inverse(A, shifts, kernel, monkeypatch, **kw):
    from gadmm_amd.ops import linalg
    for k in ("GADMM_INV_REG", "GADMM_GJ64", "GADMM_BIGINV"):
        monkeypatch.delenv(k, raising=False)
    for k, v in SMALL_KERNELS[kernel].items():
        monkeypatch.setenv(k, v)
    (n, v), d = shifts.shape, A.shape[-1]
    out = _nan(n, v, d, d)
    res = linalg.spd_inverse(_dev(A), _dev(shifts), out=out, **kw)
    assert res.data_ptr() == out.data_ptr()
    return _host(out)


def _check_inverse(tag, case, out, nb=None, skip=()):
    good = np.array([[(n, v) not in skip for v in range(out.shape[1])] for n in range(out.shape[0])])
    assert not np.isnan(out[good]).any(), "an output element was not written"
    assert np.array_equal(out[good], out[good].transpose(0, 2, 1)), "the inverse is not exactly symmetric"
    _report(tag, case.ratios(out, nb, skip))


def _kinds(d):
    return [k for k in H.INVERSE_KINDS if not (k == "ill" and d < 2)]  # a 1 x 1 matrix has kappa 1


# d <= 64: 1, 2 (one lane live), 7, 8, 9 (the register kernel keeps columns w + 8 c per wave), 63, 64.
@pytest.mark.parametrize("d", H.INV_SMALL_D)
def test_spd_inverse_small_kernels(d, monkeypatch):
    for kind in _kinds(d):
        case = H.inverse_case(kind, d)
        outs = {}
        for kernel in SMALL_KERNELS:
            outs[kernel] = _small_inverse(case.A, case.shifts, kernel, monkeypatch)
            _check_inverse("inverse %s %s d %d" % (kernel, kind, d), case, outs[kernel])
        assert np.array_equal(outs["register"], outs["general"]) and np.array_equal(outs["lds64"], outs["general"]), \
            "the d <= 64 kernels are not bit-identical (%s, d = %d)" % (kind, d)


# the general kernel alone: 32 / 33 its 256 / 1024-thread switch; every d > 64; 90 / 91 the last d within
# 64 KB of dynamic LDS and the first past it; 127, 128 the top.
@pytest.mark.parametrize("d", H.INV_GENERAL_D)
def test_spd_inverse_general_kernel(d, monkeypatch):
    for kind in _kinds(d):
        case = H.inverse_case(kind, d)
        _check_inverse("inverse general %s d %d" % (kind, d), case,
                       _small_inverse(case.A, case.shifts, "general", monkeypatch))


# (d) blocked inverse: 129 = 128 + 1 / 64 + 64 + 1; 192 = 128 + 64 / 3 x 64; 193 (nb = 128: a 65-wide
# last block, which recurses into 64 + 1); 257 (a 1-wide last block). One matrix: the single-stream
# launch; four: odd matrices on the side stream with the second workspace half.
def _blocked_inverse(A, shifts, nb, **kw):
    from gadmm_amd.ops import linalg
    (n, v), d = shifts.shape, A.shape[-1]
    out = _nan(n, v, d, d)
    res = linalg.spd_inverse_blocked(_dev(A), torch.from_numpy(np.ascontiguousarray(shifts)), out=out, nb=nb, **kw)
    assert res.data_ptr() == out.data_ptr()
    return _host(out)


@pytest.mark.parametrize("d", H.INV_BLOCKED_D)
@pytest.mark.parametrize("nb", [64, 128])
@pytest.mark.parametrize("kind", H.INVERSE_KINDS)
@pytest.mark.parametrize("workers,variants", [(1, 1), (2, 2)])
def test_spd_inverse_blocked(kind, d, nb, workers, variants):
    case = H.inverse_case(kind, d, workers=workers, variants=variants)
    _check_inverse("inverse blocked nb %d %s d %d x%d" % (nb, kind, d, workers * variants), case,
                   _blocked_inverse(case.A, case.shifts, nb), nb)


# ------------------------------------------------------------------------------------------------
# (e) the status word
def _status_case(d, bad, nan):
    """Three well-conditioned matrices (one variant each); worker 1's is replaced by a matrix whose
    Gauss-Jordan pivot first turns non-positive (or NaN) at index ``bad``."""
    case = H.inverse_case("well", d, workers=3, variants=1)
    A = np.array(case.A)
    A[1] = d * H.non_spd_matrix(d, bad, nan=nan) - case.shifts[1, 0] * np.eye(d)
    return case, A


def _word():
    return torch.zeros((1,), dtype=torch.int32, device=DEV)


def _status_protocol(tag, case, A, run, nb=None):
    """``run(A, shifts, **kw) -> out`` on (3, d, d): raises on the bad matrix; with a caller's word the
    word reads 1 and the two good matrices still meet their bound; the word stays 1 over an SPD call;
    a fresh word after an SPD call reads 0."""
    with pytest.raises(FloatingPointError):
        run(A, case.shifts)
    w = _word()
    out = run(A, case.shifts, check_status=False, status=w)
    assert int(w.item()) == 1, "%s: the status word is not set" % tag
    _check_inverse(tag + " (beside a non-SPD matrix)", case, out, nb, skip={(1, 0)})
    good = run(case.A, case.shifts, check_status=False, status=w)
    assert int(w.item()) == 1, "%s: the status word is not sticky" % tag
    _check_inverse(tag + " (SPD, set word)", case, good, nb)
    w2 = _word()
    run(case.A, case.shifts, check_status=False, status=w2)
    assert int(w2.item()) == 0, "%s: SPD input set the status word" % tag
    run(case.A, case.shifts)  # and does not raise


@pytest.mark.parametrize("d", [9, 64])
@pytest.mark.parametrize("kernel", list(SMALL_KERNELS))
@pytest.mark.parametrize("where", ["first", "middle", "last", "nan"])
def test_spd_inverse_status_word(where, kernel, d, monkeypatch):
    bad = {"first": 0, "middle": d // 2, "last": d - 1, "nan": d // 3}[where]
    case, A = _status_case(d, bad, where == "nan")

    def run(A_, shifts, **kw):
        return _small_inverse(A_, shifts, kernel, monkeypatch, **kw)
    _status_protocol("status %s %s d %d" % (kernel, where, d), case, A, run)


# d = 200, the bad pivot at index 150: nb = 128 -> inside the 72-wide last block, which recurses into
# 64 + 8 (index 22 of its first block); nb = 64 -> inside the third block. One matrix (the single
# stream) and three (the bad one on the side stream).
@pytest.mark.parametrize("nb", [64, 128])
@pytest.mark.parametrize("where", ["pivot", "nan"])
def test_spd_inverse_blocked_status_word(where, nb):
    from gadmm_amd.ops import linalg
    d, bad = 200, 150
    case, A = _status_case(d, bad, where == "nan")

    def run(A_, shifts, **kw):
        return _blocked_inverse(A_, shifts, nb, **kw)
    _status_protocol("status blocked nb %d %s d %d x3" % (nb, where, d), case, A, run, nb)
    # one matrix, the single-stream launch
    one = (A[1:2], case.shifts[1:2])
    with pytest.raises(FloatingPointError):
        run(*one)
    w = _word()
    run(*one, check_status=False, status=w)
    assert int(w.item()) == 1
    w = _word()
    out = run(case.A[:1], case.shifts[:1], check_status=False, status=w)
    assert int(w.item()) == 0
    single = H.inverse_case("well", d, workers=1, variants=1)
    assert single.mats[0][0] is case.mats[0][0]
    _check_inverse("status blocked nb %d %s d %d x1 (SPD)" % (nb, where, d), single, out, nb)
    with pytest.raises(FloatingPointError):  # linalg.spd_inverse routes d > 128 to the blocked kernel
        linalg.spd_inverse(_dev(A[1:2]), _dev(case.shifts[1:2]))
