"""The posterior Exp(1) noise of include/var_hip.h ("posterior Exp(1) noise given the drawn token"), restated in numpy float32
from the header's text.  No line here is taken from abduct.hip: the repair in particular is not the kernel's closed form plus steps but the
definition itself — the smallest float at or above the candidate whose score is strictly below the winner's — found by bisection on the
float's bit pattern (scores do not increase with the noise, positive floats order as their bit patterns do).

Primitives: the Exp(1) stream comes from the library's host fill (varhip_exp1_philox_host_f32, pinned by tests/test_per_image_cpu.py),
vm_exp from tests/codecref.py's restatement (pinned there), vm_log is restated below the same way, one operation at a time."""
import numpy as np

from tests.codecref import _fma32, vm_exp

F = np.float32
FLT_MIN = F(1.17549435e-38)
DRAW_FILL, DRAW_MIN = 2, 3


def vm_log(x):
    """include/var_math.h's vm_log on a binary32 array of normal positive numbers"""
    x = np.asarray(x, F)
    assert bool(((x >= FLT_MIN) & np.isfinite(x)).all())
    u = x.view(np.uint32)
    fe = ((u >> np.uint32(23)).astype(np.int32) - 126).astype(F)
    m = ((u & np.uint32(0x007fffff)) | np.uint32(0x3f000000)).view(F)
    low = m < F(0.707106781186547524)
    fe = np.where(low, fe - F(1.0), fe).astype(F)
    m = np.where(low, ((m + m).astype(F) - F(1.0)).astype(F), (m - F(1.0)).astype(F)).astype(F)
    z = (m * m).astype(F)
    p = np.full(x.shape, F(7.0376836292e-2), F)
    for c in (-1.1514610310e-1, 1.1676998740e-1, -1.2420140846e-1, 1.4249322787e-1, -1.6668057665e-1, 2.0000714765e-1, -2.4999993993e-1,
              3.3333331174e-1):
        p = _fma32(p, m, F(c))
    y = ((p * m).astype(F) * z).astype(F)
    y = _fma32(F(-2.12194440e-4), fe, y)
    y = _fma32(F(-0.5), z, y)
    return _fma32(F(0.693359375), fe, (m + y).astype(F))


def canon_sum256(e):
    """the sampler's row sum of (R, V) float32: thread i of 256 adds its elements i, i + 256, ... in ascending order from 0, a wave of 64
    threads is summed by the xor butterfly 32, 16, 8, 4, 2, 1, the four waves as ((w0 + w1) + w2) + w3"""
    R, V = e.shape
    pad = (-V) % 256
    e = np.concatenate((e, np.zeros((R, pad), F)), axis=1) if pad else e
    part = np.zeros((R, 256), F)
    for k in range(e.shape[1] // 256):
        part = (part + e[:, 256 * k:256 * k + 256]).astype(F)
    w = part.reshape(R, 4, 64)
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = (w + w[:, :, lanes ^ off]).astype(F)
    w = w[:, :, 0]
    return (((w[:, 0] + w[:, 1]).astype(F) + w[:, 2]).astype(F) + w[:, 3]).astype(F)


def stream(seeds, l, V, scale, draw):
    """(B * l, V) of the project's Exp(1) stream"""
    from var_amd import hip
    seeds = np.ascontiguousarray(seeds, np.int64)
    out = np.full((len(seeds) * l, V), np.nan, F)
    hip.call_host('exp1_philox_host_f32', seeds, len(seeds), l, V, scale, draw, out)
    return out


def guided(logits, B, l, t):
    """logits (2 * B * l, V), t (B,) float64 -> x (B * l, V): ca * cond - cb * uncond, three roundings"""
    rows = B * l
    tt = np.repeat(np.asarray(t, np.float64), l)
    ca, cb = (1.0 + tt).astype(F)[:, None], tt.astype(F)[:, None]
    with np.errstate(all='ignore'):
        return ((ca * logits[:rows]).astype(F) - (cb * logits[rows:]).astype(F)).astype(F)


def probabilities(x):
    """-> (p (R, V), m (R,), S (R,)) of the guided rows, as the sampler's last stage forms them without a filter"""
    with np.errstate(all='ignore'):
        m = np.fmax.reduce(x, axis=1)
        ev = vm_exp((x - m[:, None]).astype(F))
        S = canon_sum256(ev)
        return (ev / S[:, None]).astype(F), m, S


def posterior(logits, t, gt, seeds, B, l, V, scale, T_zero=False, drop_E=False):
    """-> (noise (B * l, V) float32, logp (B * l,) float32, flag (B * l,) int32).  gt: (B * l,) tokens.  T_zero / drop_E: planted faults for the
    law test (the minimum's draw replaced by 0; the fresh fill left out of the losers' candidates)."""
    rows = B * l
    gt = np.asarray(gt, np.int64).reshape(rows)
    x = guided(np.asarray(logits, F).reshape(2 * rows, V), B, l, t)
    p, m, S = probabilities(x)
    E = stream(seeds, l, V, scale, DRAW_FILL)
    T = stream(seeds, l, V, scale, DRAW_MIN)[:, 0].copy()
    if T_zero:
        T[:] = 0
    valid = (gt >= 0) & (gt < V)
    g = np.where(valid, gt, 0)
    r = np.arange(rows)
    pg = p[r, g]
    with np.errstate(all='ignore'):
        ng = np.maximum((T * pg).astype(F), FLT_MIN)
        rg = (pg / ng).astype(F)
        flag = ~valid | np.isnan(x).any(axis=1) | (pg == 0) | ~(np.isfinite(rg) & (rg > 0))
        cand = ((T[:, None] * p).astype(F) + (F(0) if drop_E else E)).astype(F)
        lo = cand.view(np.uint32).astype(np.int64)                                  # the smallest admissible pattern lies in [lo, hi]
        hi = np.full(lo.shape, 0x7f7fffff, np.int64)
        loses = lambda bits: (p / bits.astype(np.uint32).view(F)).astype(F) < rg[:, None]
        live = ~flag[:, None] & np.ones_like(lo, bool)
        if not drop_E:
            assert bool(loses(hi)[live].all())
        done = loses(lo)
        hi = np.where(done, lo, hi)
        for _ in range(32):
            mid = (lo + hi) // 2
            ok = loses(mid)
            hi = np.where(ok, mid, hi)
            lo = np.where(ok, lo, np.minimum(mid + 1, hi))
        noise = hi.astype(np.uint32).view(F).copy()
    noise[r, g] = ng
    noise[flag] = E[flag]
    with np.errstate(all='ignore'):
        Ssafe = np.where(flag, F(1.0), S)
        logp = ((x[r, g] - m).astype(F) - vm_log(Ssafe)).astype(F)
    logp[flag] = -np.inf
    return noise, logp, flag.astype(np.int32)
