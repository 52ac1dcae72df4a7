"""A plain numpy / Python restatement of varhip_smc_resample_f32's contract (include/var_hip.h, steps 1 to 7), written from that text: Python
floats are IEEE binary64 and every sum below is a loop in the stated order, so the result is what the contract says bit for bit.  The one
binary32 function involved, vm_exp of include/var_math.h, is restated from its description with an exactly rounded fma (rational arithmetic,
then one rounding to binary32).  Also here: Philox4x32-10 from the paper's round function and the Random123 known answers it is held to."""
from fractions import Fraction

import numpy as np

# the published known-answer vectors of philox4x32_10 (Random123 kat_vectors): (counter, key, output)
PHILOX_KAT = [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]
M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox4x32-10 on Python integers"""
    c0, c1, c2, c3 = [int(c) & M32 for c in ctr]
    k0, k1 = [int(k) & M32 for k in key]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return [c0, c1, c2, c3]


def uniform(seed: int, scale: int) -> float:
    """step 6's u: word 0 of Philox with the seed's low and high words as the key and the counter (0, 0, scale, 2)"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x = philox4x32_10([0, 0, scale, 2], [seed & M32, seed >> 32])[0]
    return (2 * (x >> 9) + 1) * 2.0 ** -24


def _rn32(x: Fraction) -> np.float32:
    """a rational rounded to binary32 once, to nearest, ties to even"""
    if x == 0:
        return np.float32(0.0)
    f = np.float32(float(x))
    cands = {f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))}
    return min(cands, key=lambda c: (abs(Fraction(float(c)) - x), int(np.float32(c).view(np.uint32)) & 1))


def _fma(a, b, c) -> np.float32:
    return _rn32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def vm_exp(x) -> np.float32:
    """include/var_math.h's vm_exp, operation by operation in binary32"""
    f = np.float32
    x = f(x)
    if np.isnan(x):
        return x
    if not x > f(-87.0):
        return f(0.0)
    if x > f(88.0):
        x = f(88.0)
    n = np.rint(f(x * f(1.44269504088896341)))
    r = _fma(n, f(-0.693145751953125), x)
    r = _fma(n, f(-1.42860682030941723212e-6), r)
    p = f(1.9875691500e-4)
    for c in (1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1):
        p = _fma(p, r, f(c))
    y = f(_fma(p, f(r * r), r) + f(1.0))
    return f(y * np.ldexp(f(1.0), int(n)))


def resample(tokens, ld_img, ld_cls, images, n, t0, t1, beta, logw, seeds, scale, ess_frac):
    """-> dict(logw, anc, did, ess, logw_seen, offspring (None where the image did not resample), w) for the flat arrays of the ABI"""
    with np.errstate(all='ignore'):
        return _resample(tokens, ld_img, ld_cls, images, n, t0, t1, float(beta), logw, seeds, scale, float(ess_frac))


def _resample(tokens, ld_img, ld_cls, images, n, t0, t1, beta, logw, seeds, scale, ess_frac):
    logw = np.array(logw, np.float64).reshape(images, n).copy()
    seen = np.empty((images, n), np.float64)
    anc = np.empty((images, n), np.int32)
    did = np.zeros(images, np.int32)
    ess = np.zeros(images, np.float64)
    offspring, weights = [None] * images, [None] * images
    tok = None if tokens is None else np.asarray(tokens, np.float32).reshape(-1)
    for i in range(images):
        for c in range(n):                                                  # step 1
            s = np.float64(0.0)
            for t in range(t0, t1):
                s = s + np.float64(tok[i * ld_img + c * ld_cls + t])
            logw[i, c] = logw[i, c] + np.float64(beta) * s
        seen[i] = logw[i]
        anc[i] = np.arange(n)
        ok = [c for c in range(n) if not np.isnan(logw[i, c])]              # step 2
        m = max((logw[i, c] for c in ok), default=np.float64(np.nan))
        if not ok or not np.isfinite(m):
            continue
        w = [np.float64(0.0) if np.isnan(logw[i, c]) else np.float64(vm_exp(np.float32(logw[i, c] - m))) for c in range(n)]      # step 3
        weights[i] = np.array(w)
        W = Q = np.float64(0.0)                                             # step 4
        for c in range(n):
            W = W + w[c]
            Q = Q + w[c] * w[c]
        ess[i] = W * W / Q
        if not (ess_frac < 0 or ess[i] < np.float64(ess_frac) * np.float64(n)):      # step 5
            continue
        u = np.float64(uniform(seeds[i], scale))                            # step 6
        step = W / np.float64(n)
        T = [(np.float64(j) + u) * step for j in range(n)]
        C, acc = [], np.float64(0.0)
        for c in range(n):
            acc = acc + w[c]
            C.append(acc)
        o = [sum(1 for j in range(n) if (C[c - 1] if c else 0.0) <= T[j] < C[c]) for c in range(n)]
        last = max(c for c in range(n) if w[c] > 0)
        o[last] += sum(1 for j in range(n) if not T[j] < C[n - 1])
        offspring[i] = np.array(o)
        dead = [c for c in range(n) if o[c] == 0]                           # step 7
        copies = [c for c in range(n) for _ in range(o[c] - 1)]
        assert len(dead) == len(copies)
        for d, c in zip(dead, copies):
            anc[i, d] = c
        logw[i] = 0.0
        did[i] = 1
    return dict(logw=logw.reshape(-1), anc=anc.reshape(-1), did=did, ess=ess, logw_seen=seen.reshape(-1), offspring=offspring, w=weights)


# ---- the cases both the host twin (tests/test_smc_resample_cpu.py) and the kernel (tests/test_smc_kernels_gpu.py) are held to ----------------
def make_case(n, beta, ess_frac, images=3, t0=2, t1=9, pad=0, scale=4, seed=0):
    """per-token statistics that look like log-probabilities (negative, a few units apart), log-weights that are not zero on entry"""
    rng = np.random.default_rng(1000 * n + 10 * int(beta) + int(10 * ess_frac) + seed + 7 * pad + t1)
    ld_cls = max(t1, 1) + pad
    ld_img = n * ld_cls + 3 * pad
    tokens = None if t1 == t0 else (-rng.gamma(2.0, 1.5, images * ld_img)).astype(np.float32)
    logw = rng.normal(0.0, 1.0, images * n)
    seeds = rng.integers(0, 2 ** 63, images, dtype=np.int64)
    return dict(tokens=tokens, ld_img=ld_img, ld_cls=ld_cls, images=images, n=n, t0=t0, t1=t1, beta=float(beta), logw=logw, seeds=seeds,
                scale=scale, ess_frac=float(ess_frac))


def cases():
    out = []
    for n in (1, 2, 3, 8, 64):
        for beta in (0, 1, 50):
            for ess_frac in (-1, 0.5, 1.0):
                out.append(make_case(n, beta, ess_frac))
    for beta, ess_frac in ((1, -1), (50, 0.5), (0, 1.0), (1, 0.5)):
        out.append(make_case(257, beta, ess_frac, images=2))
    out.append(make_case(8, 1, -1, t0=5, t1=5))              # t1 == t0: NULL tokens, the weights are ranked as given
    out.append(make_case(3, 1, 0.5, t0=0, t1=0, scale=0))
    out.append(make_case(8, 1, -1, pad=5))                   # a padded ld_cls (and ld_img)
    out.append(make_case(64, 1, 0.5, pad=3, t0=0, t1=30, scale=6))
    return out


def case_id(c):
    return f"n{c['n']}-b{c['beta']:g}-e{c['ess_frac']:g}-t{c['t0']}_{c['t1']}-ld{c['ld_cls']}"


def ref_of(c):
    return resample(c['tokens'], c['ld_img'], c['ld_cls'], c['images'], c['n'], c['t0'], c['t1'], c['beta'], c['logw'], c['seeds'], c['scale'],
                    c['ess_frac'])


def call_args(c, out):
    """the ABI's argument list for case c with the output arrays of `out` (logw is in and out: out['logw'] starts as a copy of c['logw'])"""
    return [c['tokens'], c['ld_img'], c['ld_cls'], c['images'], c['n'], c['t0'], c['t1'], c['beta'], out['logw'], c['seeds'], c['scale'],
            c['ess_frac'], out['anc'], out['did'], out['ess'], out['logw_seen']]


def fresh_outputs(c, seen=True):
    N, images = max(c['images'] * c['n'], 1), max(c['images'], 1)        # (an argument list that is refused may carry sizes below 1)
    return dict(logw=np.array(c['logw'], np.float64).copy(), anc=np.full(N, -7, np.int32), did=np.full(images, -7, np.int32),
                ess=np.full(images, -7.0, np.float64), logw_seen=np.full(N, -7.0, np.float64) if seen else None)


FIELDS = ('anc', 'did', 'ess', 'logw', 'logw_seen')


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
