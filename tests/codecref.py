"""The coding table and the rANS coder of include/var_hip.h ("lossless token coding"), restated from the header's text in numpy fp32 for the
part that is floating point (z, m, e) and in plain Python integers for everything behind it.  No line here is taken from codec.hip.

vm_exp: include/var_math.h's operations one by one.  A binary32 fma is evaluated in float64: the product of two binary32 values is exact
there, the sum is made round-to-odd with the addition's exact error (TwoSum), and a round-to-odd 53-bit value rounds to binary32 as the exact
one does (53 >= 24 + 2)."""
import bisect

import numpy as np

PB = 24
TOTAL = 1 << PB
LOW = 1 << 31
F32 = np.float32


def _fma32(a, b, c):
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64) if s.ndim else np.array(s).view(np.int64)
    even = (bits & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & even, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def vm_exp(x):
    """include/var_math.h's vm_exp on a binary32 array"""
    x = np.asarray(x, np.float32)
    with np.errstate(all='ignore'):
        xc = np.where(x > F32(88.0), F32(88.0), x)
        xc = np.where(x > F32(-87.0), xc, F32(0.0))              # (placeholder where the result is 0 or NaN anyway)
        n = np.rint((xc * F32(1.44269504088896341)).astype(np.float32)).astype(np.float32)
        r = _fma32(n, F32(-0.693145751953125), xc)
        r = _fma32(n, F32(-1.42860682030941723212e-6), r)
        p = np.full(x.shape, F32(1.9875691500e-4), np.float32)
        for c in (1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1):
            p = _fma32(p, r, F32(c))
        y = (_fma32(p, (r * r).astype(np.float32), r) + F32(1.0)).astype(np.float32)
        out = (y * np.ldexp(F32(1.0), n.astype(np.int32)).astype(np.float32)).astype(np.float32)
        out = np.where(x > F32(-87.0), out, F32(0.0))
        return np.where(np.isnan(x), x, out).astype(np.float32)


def guided(cond, uncond, t):
    """z = ca * cond - cb * uncond, three binary32 roundings"""
    ca, cb = F32(1.0 + float(t)), F32(float(t))
    with np.errstate(all='ignore'):
        a = (ca * np.asarray(cond, np.float32)).astype(np.float32)
        b = (cb * np.asarray(uncond, np.float32)).astype(np.float32)
        return (a - b).astype(np.float32)


def table(z):
    """-> (F list of V Python ints, v*) of one guided row z, or None where the row is refused"""
    z = np.asarray(z, np.float32)
    V = z.shape[0]
    if np.isnan(z).any():
        return None
    m = z.max()
    if np.isinf(m):
        return None
    with np.errstate(all='ignore'):
        e = vm_exp((z - m).astype(np.float32))
    i = [int(np.floor(np.float64(ev) * 4294967296.0)) for ev in e]
    I = sum(i)
    K = TOTAL - V
    q = [(iv * K) // I for iv in i]
    D = K - sum(q)
    assert 0 <= D < V
    vstar = int(np.flatnonzero(z == m)[0])
    F = [1 + qv for qv in q]
    F[vstar] += D
    return F, vstar


def tables(logits, B, l, t_of_image):
    """logits (2 * B * l, V) -> [per row: (F, v*) | None]"""
    rows = B * l
    return [table(guided(logits[w], logits[rows + w], t_of_image[w // l])) for w in range(rows)]


def cumulative(F):
    """the inclusive cumulative table"""
    out, c = [], 0
    for f in F:
        c += f
        out.append(c)
    return out


def encode(pairs):
    """[(C, F)] in token order -> the stream, a list of 32-bit words"""
    x = LOW
    emitted = []
    for C, F in reversed(pairs):
        if x >= ((LOW >> PB) << 32) * F:
            emitted.append(x & 0xFFFFFFFF)
            x >>= 32
        x = ((x // F) << PB) + x % F + C
    return [x >> 32, x & 0xFFFFFFFF] + emitted[::-1]


def decode(cums, words):
    """cums: per token the inclusive table -> (tokens with -1 from an error on, err, x, words consumed)"""
    toks, err = [], 0
    if len(words) < 2:
        return [-1] * len(cums), 1, 0, 0
    x, pos = (words[0] << 32) | words[1], 2
    for cum in cums:
        if err:
            toks.append(-1)
            continue
        slot = x & (TOTAL - 1)
        s = bisect.bisect_right(cum, slot)                      # the first entry above the slot (the table ascends)
        if s == len(cum):
            err = 2
            toks.append(-1)
            continue
        C = cum[s - 1] if s else 0
        x = (cum[s] - C) * (x >> PB) + slot - C
        toks.append(s)
        if x < LOW:
            if pos >= len(words):
                err = 1
            else:
                x = (x << 32) | words[pos]
                pos += 1
    return toks, err, x, pos


def ideal_bits(Fs):
    return float(sum(PB - np.log2(float(f)) for f in Fs))
