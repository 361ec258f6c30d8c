"""Q-GADMM stochastic quantizer (Elgabli et al., arXiv:1910.10453): the specification every layer
(torch path, graph-engine phase kernel, persistent kernel) reproduces bit for bit.

A worker keeps a public model ``th_hat`` that its chain neighbours hold an identical copy of. After
solving for ``theta`` in iteration ``it`` (1-based) worker ``w`` sends the quantized difference to it,
``bits`` per coordinate. With ``L = 2^bits - 1`` and every operation a separately rounded IEEE f64
operation (no FMA contraction)::

    diff_i = theta_i - th_hat_i          R = max_i |diff_i|
    R == 0:  q_i = 0, th_hat unchanged
    else     delta = (2.0 * R) / L       c_i = (diff_i + R) / delta
             q_i = clamp(floor(c_i + u_i), 0, L)
             th_hat_i <- th_hat_i + (q_i * delta - R)

``u_i`` is a counter-based uniform (splitmix64 finaliser of a Weyl sequence, integers mod 2^64)::

    x = seed + 0x9e3779b97f4a7c15 * (((it * N + w) * d + i) + 1)
    z = x;  z = (z ^ z >> 30) * 0xbf58476d1ce4e5b9;  z = (z ^ z >> 27) * 0x94d049bb133111eb;  z ^= z >> 31
    u = (z >> 11) * 2^-53

The message is ``(R, q_0 .. q_{d-1})``: ``bits * d + 64`` payload bits instead of ``64 * d``. A
receiver applies the last line (``dequantize``) to its copy. On the wire the codes are packed
``64 / bits`` per 64-bit word, coordinate ``i`` at bit ``bits * (i mod 64/bits)`` of word
``i // (64/bits)`` (``pack_codes`` / ``unpack_codes``).

The quantizer also reports a *flip margin*: the minimum over the coordinates whose code is not at an
end of the range of ``min(frac(c + u), 1 - frac(c + u)) * delta / max|theta|`` -- how far, relative to
the iterate, the nearest rounding decision is from going the other way (the idiom of the LAG
``trigger_margin``). A comparison of two implementations of a quantized run means something only while
it stays well above their rounding differences.

Censoring (C-GADMM / CQ-GGADMM, Ben Issaid et al., arXiv:2009.06459) sits on top of the quantizer and
changes nothing in it: a worker transmits only when its public model would move by at least a
geometrically decaying threshold. With ``cand`` the new public model ``quantize_rows`` proposes for
worker ``w`` at iteration ``it`` (1-based), every line one rounded IEEE f64 operation (no FMA)::

    step_i = cand_i - th_hat_i           sq_i = step_i * step_i           s = sum64(sq)
    thr_0  = tau0;  thr_k = thr_{k-1} * xi                                thr2[k] = thr_k * thr_k
    send   = s >= thr2[it]
    send:      th_hat <- cand, the message (R, codes) as above
    not send:  th_hat unchanged, nothing travels but a one-word "censored" notice

``sum64`` is the order the kernels sum in: pad with zeros to a multiple of 64, on each 64-chunk run
the butterfly ``x <- x + x[i ^ off]`` for ``off = 32, 16, 8, 4, 2, 1`` and take element 0, then add
the chunks' results in order, starting from 0.0. ``tau0 = 0`` gives ``thr2 == 0``: every worker always
sends, and the run is Q-GADMM bit for bit. ``R == 0`` gives ``s = 0``: censored whenever
``thr2 > 0``. The *censor margin* is the minimum over the decisions with ``thr2 > 0`` of
``|s - thr2| / thr2``: two implementations can be compared only while it stays well above their
rounding differences (the idiom of the flip margin).
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

BITS = (4, 8, 16)
_GOLDEN = 0x9e3779b97f4a7c15
_M1 = 0xbf58476d1ce4e5b9
_M2 = 0x94d049bb133111eb
_MASK = (1 << 64) - 1
# header word of a censored message where a message's first word holds the bits of R: the sign bit,
# which no R = max |diff| >= 0 carries
CENSORED_HEADER = 1 << 63


def check_bits(bits) -> int:
    """``bits`` as an int if the quantizer offers it (2 diverges at the reference's rho; see README)."""
    if int(bits) != bits or int(bits) not in BITS:
        raise ValueError("Q-GADMM: bits must be one of %s, got %r" % (BITS, bits))
    return int(bits)


def u01(seed: int, it: int, n_workers: int, w, d: int) -> np.ndarray:
    """The ``d`` uniforms in [0, 1) of worker(s) ``w`` (an id, or an array of ids: one row each) at
    iteration ``it`` of an ``n_workers``-worker solve."""
    w_arr = np.asarray(w, dtype=np.int64)
    with np.errstate(over="ignore"):
        base = np.uint64(int(it) * int(n_workers)) + w_arr.astype(np.uint64)
        idx = base[..., None] * np.uint64(d) + np.arange(d, dtype=np.uint64) + np.uint64(1)
        z = np.uint64(int(seed) & _MASK) + np.uint64(_GOLDEN) * idx
        z = (z ^ (z >> np.uint64(30))) * np.uint64(_M1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(_M2)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def dequantize(th_hat: np.ndarray, R, q: np.ndarray, bits: int) -> np.ndarray:
    """A receiver's update of its copy ``th_hat`` (..., d) from the message ``(R (...), q (..., d))``."""
    L = float((1 << int(bits)) - 1)
    th_hat = np.asarray(th_hat, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)[..., None]
    with np.errstate(invalid="ignore", divide="ignore"):
        delta = (2.0 * R) / L
        new = th_hat + (np.asarray(q).astype(np.float64) * delta - R)
    return np.where(R == 0.0, th_hat, new)


def quantize_rows(theta: np.ndarray, th_hat: np.ndarray, bits: int, u: np.ndarray
                  ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, float]:
    """Quantize rows ``theta`` (k, d) against the public models ``th_hat`` (k, d) with the uniforms
    ``u`` (k, d): ``(R (k,), q (k, d) int64, new th_hat (k, d), flip margin)``; the margin is ``inf``
    when no coordinate has an interior code."""
    bits = check_bits(bits)
    L = float((1 << bits) - 1)
    theta = np.asarray(theta, dtype=np.float64)
    th_hat = np.asarray(th_hat, dtype=np.float64)
    diff = theta - th_hat
    R = np.max(np.abs(diff), axis=-1)
    Rc = R[..., None]
    with np.errstate(invalid="ignore", divide="ignore"):
        delta = (2.0 * Rc) / L
        c = (diff + Rc) / delta
        s = c + u
        fl = np.floor(s)
    live = Rc != 0.0
    q = np.where(live, np.clip(np.where(np.isfinite(fl), fl, 0.0), 0.0, L), 0.0).astype(np.int64)
    new = dequantize(th_hat, R, q, bits)
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = s - fl
        m = np.minimum(frac, 1.0 - frac) * delta / np.max(np.abs(theta), axis=-1)[..., None]
    interior = live & (q > 0) & (q < int(L)) & np.isfinite(m)
    margin = float(np.min(m[interior])) if np.any(interior) else float("inf")
    return R, q, new, margin


def quantize_row(theta: np.ndarray, th_hat: np.ndarray, bits: int, u: np.ndarray):
    """One worker's message: ``(R, q (d,), new th_hat (d,), flip margin)``."""
    R, q, new, margin = quantize_rows(np.asarray(theta)[None], np.asarray(th_hat)[None], bits, np.asarray(u)[None])
    return float(R[0]), q[0], new[0], margin


def words_per_row(d: int, bits: int) -> int:
    """64-bit code words of one message: ``ceil(d * bits / 64)``."""
    per = 64 // check_bits(bits)
    return (int(d) + per - 1) // per


def granules_per_row(d: int, bits: int) -> int:
    """16-byte hand-off granules of one message on the native engines: one for R, one per code word."""
    return words_per_row(d, bits) + 1


def payload_bits(d: int, bits: int) -> int:
    """Payload of one transmission: ``bits * d + 64`` (the codes and R) instead of ``64 * d``."""
    return check_bits(bits) * int(d) + 64


def pack_codes(q: np.ndarray, bits: int) -> np.ndarray:
    """Codes (..., d) -> words (..., ceil(d * bits / 64)) uint64."""
    bits = check_bits(bits)
    q = np.asarray(q)
    per = 64 // bits
    d = q.shape[-1]
    nw = words_per_row(d, bits)
    if np.any(q < 0) or np.any(q > (1 << bits) - 1):
        raise ValueError("codes outside [0, 2^bits - 1]")
    pad = np.zeros(q.shape[:-1] + (nw * per,), dtype=np.uint64)
    pad[..., :d] = q.astype(np.uint64)
    sh = (np.arange(per, dtype=np.uint64) * np.uint64(bits))
    return np.bitwise_or.reduce(pad.reshape(q.shape[:-1] + (nw, per)) << sh, axis=-1)


def unpack_codes(words: np.ndarray, bits: int, d: int) -> np.ndarray:
    """Words (..., nw) uint64 -> codes (..., d) int64."""
    bits = check_bits(bits)
    per = 64 // bits
    w = np.asarray(words, dtype=np.uint64)
    sh = (np.arange(per, dtype=np.uint64) * np.uint64(bits))
    q = (w[..., None] >> sh) & np.uint64((1 << bits) - 1)
    return q.reshape(w.shape[:-1] + (-1,))[..., :int(d)].astype(np.int64)


def check_censor(censor) -> Tuple[float, float]:
    """``(tau0, xi)`` as floats if they are a censoring rule: ``tau0 >= 0`` and ``0 < xi < 1``."""
    if censor is None or len(censor) != 2:
        raise ValueError("censor: (tau0, xi)")
    tau0, xi = float(censor[0]), float(censor[1])
    if not tau0 >= 0.0 or not np.isfinite(tau0):
        raise ValueError("censor: tau0 must be finite and >= 0, got %r" % (censor[0],))
    if not 0.0 < xi < 1.0:
        raise ValueError("censor: xi must lie in (0, 1), got %r" % (censor[1],))
    return tau0, xi


def censor_thresholds(tau0: float, xi: float, n_iter: int) -> np.ndarray:
    """The table ``thr2[0 .. n_iter]`` of squared thresholds: ``thr_0 = tau0``, ``thr_k = thr_{k-1} *
    xi`` (one rounded multiply per iteration), ``thr2[k] = thr_k * thr_k``. Iteration ``it`` (1-based)
    compares with ``thr2[it]``. Computed once on the host and handed to the kernels."""
    tau0, xi = check_censor((tau0, xi))
    thr = np.empty(int(n_iter) + 1, dtype=np.float64)
    t = np.float64(tau0)
    for k in range(thr.size):
        thr[k] = t
        t = t * np.float64(xi)
    return thr * thr


def sum64(v: np.ndarray) -> np.ndarray:
    """Sum over the last axis in the order of the kernels' ``wave_sum_f64`` / ``block_sum_f64``."""
    v = np.asarray(v, dtype=np.float64)
    n = v.shape[-1]
    nc = max((n + 63) // 64, 1)
    x = np.zeros(v.shape[:-1] + (nc * 64,), dtype=np.float64)
    x[..., :n] = v
    x = x.reshape(v.shape[:-1] + (nc, 64))
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        x = x + x[..., idx ^ off]
    total = np.zeros(v.shape[:-1], dtype=np.float64)
    for c in range(nc):
        total = total + x[..., c, 0]
    return total


def censor_rows(cand: np.ndarray, th_hat: np.ndarray, thr2) -> Tuple[np.ndarray, np.ndarray, float]:
    """The censoring decision of rows ``cand`` (k, d), the public models ``quantize_rows`` proposes,
    against the current ones ``th_hat`` (k, d) under the squared threshold(s) ``thr2`` (a scalar or
    (k,)): ``(send (k,) bool, s (k,), censor margin)``; the margin is ``inf`` where ``thr2 == 0``."""
    cand = np.asarray(cand, dtype=np.float64)
    th_hat = np.asarray(th_hat, dtype=np.float64)
    step = cand - th_hat
    s = sum64(step * step)
    t2 = np.broadcast_to(np.asarray(thr2, dtype=np.float64), s.shape)
    send = s >= t2
    live = t2 > 0.0
    margin = float(np.min(np.abs(s[live] - t2[live]) / t2[live])) if np.any(live) else float("inf")
    return send, s, margin
