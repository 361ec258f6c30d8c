"""Q-GADMM on the CPU: the quantizer specification (algorithms/quantize.py) against known answers and
its properties, and the torch path of ``chain_admm(..., quantize=(bits, seed))``.

The known answers (uniforms, codes, th_hat bits, iteration counts) come from an independent
prototype of the specification; they are not re-pinned from this code.
"""
import numpy as np
import pytest
import torch

from gadmm_amd.algorithms import quantize as Q
from gadmm_amd.algorithms import group_admm_closed_form, quantized_group_admm, chain_admm

U_IT1_W0 = ["0x1.f5e3370c69fd2p-2", "0x1.67d738842ed86p-1", "0x1.37ebdeaf875efp-1", "0x1.73f551c0267b1p-1"]
U_IT3_W5 = ["0x1.13f5766d04850p-1", "0x1.acdde01a96e90p-2", "0x1.60755fe1b098ep-1", "0x1.4af3064c4c51ep-1"]
THETA = np.array([0.5, -0.25, 0.125, 1.0])
HAT = np.array([0.0, 0.25, 0.125, 0.0])
KNOWN = {
    4: ((11, 4, 8, 15), ["0x1.ddddddddddddcp-2", "-0x1.bbbbbbbbbbbbcp-3", "0x1.8888888888888p-3", "0x1p+0"]),
    8: ((191, 64, 128, 255), ["0x1.fdfdfdfdfdfe0p-2", "-0x1.fbfbfbfbfbfc0p-3", "0x1.0808080808080p-3", "0x1p+0"]),
    16: ((49151, 16384, 32768, 65535), None),
}


def _hex(v):
    return [float.fromhex(h) for h in v]


def test_u01_known_answers():
    assert Q.u01(1234, 1, 8, 0, 4).tolist() == _hex(U_IT1_W0)
    assert Q.u01(1234, 3, 8, 5, 4).tolist() == _hex(U_IT3_W5)
    both = Q.u01(1234, 3, 8, [0, 5], 4)  # rows of several workers == one call each
    assert both.shape == (2, 4) and both[1].tolist() == _hex(U_IT3_W5)
    assert both[0].tolist() == Q.u01(1234, 3, 8, 0, 4).tolist()


@pytest.mark.parametrize("bits", [4, 8, 16])
def test_quantize_known_answers(bits):
    u = np.array(_hex(U_IT1_W0))
    R, q, new, margin = Q.quantize_row(THETA, HAT, bits, u)
    codes, hat_hex = KNOWN[bits]
    assert R == 1.0
    assert tuple(q.tolist()) == codes
    if hat_hex is not None:
        assert new.tolist() == _hex(hat_hex)
    assert np.array_equal(Q.dequantize(HAT, R, q, bits), new)  # the receiver's line gives the sender's bits
    assert 0.0 < margin < 0.5 * (2.0 / ((1 << bits) - 1))


@pytest.mark.parametrize("bits", [4, 8, 16])
@pytest.mark.parametrize("d", [1, 7, 50, 64])
def test_pack_unpack_round_trip(bits, d):
    rng = np.random.default_rng(100 * bits + d)
    q = rng.integers(0, 1 << bits, size=(3, d))
    q[0, 0], q[1, -1] = (1 << bits) - 1, 0
    w = Q.pack_codes(q, bits)
    per = 64 // bits
    assert w.dtype == np.uint64 and w.shape == (3, (d + per - 1) // per) == (3, Q.words_per_row(d, bits))
    assert np.array_equal(Q.unpack_codes(w, bits, d), q)
    for i in (0, d // 2, d - 1):  # coordinate i at bit bits * (i mod per) of word i // per
        assert (int(w[2, i // per]) >> (bits * (i % per))) & ((1 << bits) - 1) == q[2, i]
    assert Q.granules_per_row(d, bits) == -(-d * bits // 64) + 1
    assert Q.payload_bits(d, bits) == bits * d + 64
    with pytest.raises(ValueError):
        Q.pack_codes(np.full((d,), 1 << bits), bits)


@pytest.mark.parametrize("bits", [4, 8, 16])
def test_quantizer_properties(bits):
    rng = np.random.default_rng(bits)
    d, L = 50, (1 << bits) - 1
    theta = rng.standard_normal((6, d))
    hat = theta + rng.standard_normal((6, d)) * np.array([1.0, 1e-3, 1e-9, 10.0, 1.0, 0.0])[:, None]
    R, q, new, margin = Q.quantize_rows(theta, hat, bits, Q.u01(7, 2, 6, np.arange(6), d))
    assert q.min() >= 0 and q.max() <= L
    assert np.array_equal(R, np.abs(theta - hat).max(axis=1))
    delta = 2.0 * R / L
    assert np.all(np.abs(new - theta).max(axis=1) <= delta)
    assert R[5] == 0.0 and np.all(q[5] == 0) and np.array_equal(new[5], hat[5])  # R = 0: unchanged
    assert margin > 0.0
    # unbiased: the mean of th_hat over 4096 seeds is within 5 standard errors of theta (plus the
    # rounding of a 4096-term f64 sum, n eps max|x|: the extremal coordinate is deterministic, se ~ 0)
    th, h0 = theta[0], hat[0]
    news = np.stack([Q.quantize_row(th, h0, bits, Q.u01(s, 1, 1, 0, d))[2] for s in range(4096)])
    se = news.std(axis=0, ddof=1) / np.sqrt(4096.0)
    dl = 2.0 * R[0] / L
    assert np.all(np.abs(news.mean(axis=0) - th) <= 5.0 * se + 4096 * np.finfo(float).eps * np.abs(news).max())
    assert np.all(news.std(axis=0) <= 0.5 * dl * 1.0001)


def test_bits_2_is_refused(lin24, lin_obj0):
    from gadmm_amd.models.linear import LinearRegression
    with pytest.raises(ValueError):
        Q.check_bits(2)
    with pytest.raises(ValueError):
        Q.quantize_row(THETA, HAT, 2, np.zeros(4))
    m = LinearRegression(lin24.X, lin24.y)
    with pytest.raises(ValueError):
        quantized_group_admm(m, 3.0, lin_obj0, 1e-4, 10, 2)


@pytest.fixture(scope="module")
def lin8():
    from gadmm_amd.data import linear_synthetic
    from gadmm_amd.models.linear import LinearRegression
    from gadmm_amd.oracle.reference import opt_linear
    ds = linear_synthetic(8)
    Xf, yf = ds.stacked()
    return LinearRegression(ds.X, ds.y), opt_linear(Xf.numpy(), yf.numpy())


@pytest.mark.parametrize("tol,iters", [(1e-4, 55), (1e-8, 93)])
def test_torch_path_counts(lin8, tol, iters):
    """linear_synthetic(8), rho = 3, b = 8, seed 1234: the prototype's iteration counts. Its gap at the
    stop / one iteration before is 0.87x / 1.17x tol (1e-4) and 0.017x / 1.21x tol (1e-8): no rounding
    flip moves the count."""
    m, obj0 = lin8
    r = quantized_group_admm(m, 3.0, obj0, tol, 500, 8, seed=1234)
    print("tol %g: iters %d gap/tol at stop %.4f before %.4f" % (tol, r.iters, r.loss[-1] / tol, r.loss[-2] / tol))
    assert r.converged and r.iters == iters
    assert r.loss[-1] < tol < r.loss[-2]
    N, d, b = 8, m.d, 8
    assert r.comm_units[-1] == r.iters * N * (b * d + 64) / (64.0 * d)
    assert np.array_equal(r.comm_units, np.arange(1, r.iters + 1) * N * (b * d + 64) / (64.0 * d))
    ex = r.extra
    assert (ex["q_bits"], ex["q_seed"], ex["payload_bits"]) == (8, 1234, r.iters * N * (b * d + 64))
    assert 0.0 < ex["min_flip_margin"] < 1.0
    assert ex["quant_fallback"] == "cpu tensors" and ex["backend"] == "torch"
    # the table holds the public models, within one quantization step of the true iterates
    th_hat, th = ex["state"][0], ex["theta_true"]
    assert th_hat.shape == th.shape and not torch.equal(th_hat, th)
    assert float((th_hat - th).abs().max()) < 1e-3


def test_quantize_none_is_the_parent_path(lin24, lin_obj0):
    """``quantize=None`` returns exactly what GADMM returns (60 iterations of lin24)."""
    from gadmm_amd.models.linear import LinearRegression
    from gadmm_amd.oracle import reference as R
    m = LinearRegression(lin24.X, lin24.y)
    a = group_admm_closed_form(m, 3.0, lin_obj0, 1e-30, 60)
    b = chain_admm(m, list(range(24)), 24, 3.0, lin_obj0, 1e-30, 60, quantize=None)
    assert a.iters == b.iters == 60
    assert np.array_equal(a.obj, b.obj) and np.array_equal(a.comm_units, b.comm_units)
    assert torch.equal(a.extra["state"][0], b.extra["state"][0]) and torch.equal(a.extra["state"][1], b.extra["state"][1])
    assert "q_bits" not in a.extra and "quant_fallback" not in b.extra
    Xn, yn = lin24.numpy()
    o = R.gadmm_linear(Xn, yn, 3.0, 60, lin_obj0, 1e-30)  # the yardstick the parent's tests use
    assert np.allclose(a.obj, o.obj, rtol=1e-11)
    assert np.array_equal(a.comm_units, np.arange(1, 61) * 24.0)


def test_quantized_run_converges_like_gadmm(lin8):
    """b = 16 tracks unquantized GADMM: same iteration count to 1e-8 on linear_synthetic(8)."""
    m, obj0 = lin8
    g = group_admm_closed_form(m, 3.0, obj0, 1e-8, 500)
    q = quantized_group_admm(m, 3.0, obj0, 1e-8, 500, 16)
    assert g.converged and q.converged and q.iters == g.iters == 93
    assert q.comm_units[-1] < 0.3 * g.comm_units[-1]


def test_quant_abi_layout_matches_ctypes():
    """The Q-GADMM fields sit at the END of PhaseArgs / PersistArgs, where the native library has them."""
    import ctypes
    from gadmm_amd.ops import native
    lib = native.require()
    buf = (ctypes.c_longlong * 16)()
    k = lib.gadmm_quant_abi_layout(buf, 16)
    PA, PS = native.PhaseArgs, native.PersistArgs
    assert list(buf[:k]) == [PA.q_true.offset, PA.q_msg.offset, PA.q_bits.offset, PA.q_seed.offset, ctypes.sizeof(PA),
                             PS.qg.offset, PS.q_true.offset, PS.q_bits.offset, PS.q_seed.offset, ctypes.sizeof(PS)]
    assert [n for n, _ in PA._fields_][-4:] == ["q_true", "q_msg", "q_bits", "q_seed"]
    assert [n for n, _ in PS._fields_][-4:] == ["qg", "q_true", "q_bits", "q_seed"]
    assert PA.q_true.offset > PA.rres.offset and PS.qg.offset > PS.ep_flush.offset
