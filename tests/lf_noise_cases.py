"""Shared by the low-frequency noise tests: a float64 oracle of the definition in include/fgc.h (fgc_synth_noise_lf),
written from that text alone on top of synth_cases.philox4x32_10 / gaussians."""
import numpy as np

import synth_cases as sc

BUMP_BIT = 0x80000000


def bump_words(K, step, seed, stream):
    """The four Philox words of every bump: counter (k, step low, step high, stream | 2^31), key seed."""
    k = np.arange(K, dtype=np.uint64)
    full = lambda v: np.full(K, v, dtype=np.uint64)
    return sc.philox4x32_10((k, full(step & sc.MASK), full((step >> 32) & sc.MASK), full((stream | BUMP_BIT) & sc.MASK)),
                            (seed & sc.MASK, seed >> 32))


def bump_table(nv, K, step, seed, stream, amplitude):
    """(centres int64 [K], amplitudes float64 [K]): c_k = (x0 nv) >> 32, a_k = A z with z the first Gaussian of (x2, x3)."""
    x = bump_words(K, step, seed, stream)
    centres = ((x[0] * np.uint64(nv)) >> np.uint64(32)).astype(np.int64)
    u0 = ((x[2] >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    u1 = ((x[3] >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    z = np.sqrt(-2.0 * np.log(u0)) * np.cos(2.0 * np.pi * u1)
    return centres, float(amplitude) * z


def field(V, centres, amps, width, chunk=256):
    """(s [nv], T [nv]) in float64 on the clean vertices V: s_i = sum_k a_k exp(-t_ik), t_ik = |v_i - v_ck|^2 / (2 w^2), and
    T_i = sum_k |a_k| (1 + t_ik) exp(-t_ik), the scale of the fp32 error."""
    V = np.asarray(V, dtype=np.float64)
    s, T = np.zeros(V.shape[0]), np.zeros(V.shape[0])
    for j in range(0, len(centres), chunk):
        c, a = V[centres[j:j + chunk]], amps[j:j + chunk]
        t = ((V[:, None, :] - c[None, :, :]) ** 2).sum(2) / (2.0 * float(width) ** 2)
        e = np.exp(-t)
        s += e @ a
        T += ((1.0 + t) * e) @ np.abs(a)
    return s, T


def field_bound(T, K, vmax):
    """The per-vertex bound of the issue: (1e-5 + (K + 16) 2^-24) T_i + 2^-23 max|V|."""
    return (1e-5 + (K + 16) * 2.0 ** -24) * T + 2.0 ** -23 * float(vmax)


def mulhi32(a, b):
    return (int(a) * int(b)) >> 32
