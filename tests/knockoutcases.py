"""The deck for varhip_attn_keysel_f32 (var_amd/csrc/attn.hip: attention over a per-(row, head) subset of the key scales), its operand builder,
the gather helper and the float64 reference, shared by tests/test_knockout_cpu.py (the yardstick proven on the CPU) and
tests/test_knockout_kernels_gpu.py (the kernel).

THE CONTRACT (include/var_hip.h): the visible keys of (row, head), in ascending cache order, form a logical sequence of n keys, and the output is
what varhip_attn_cached_f32 computes on a cache that holds exactly those keys at 0 .. n - 1 with curL = n, bit for bit.  So the twin of the new
kernel is "gather, then the existing kernel" (on the GPU) or "gather, then the oracle's attn_cached_f32" (on the CPU): gather() below.  What
keeps gather() honest is masked_reference(): float64 softmax(q k^T) v over the visible keys, taken from the UNGATHERED cache with a boolean key
mask, and the derived bar of tests/attncases.py with n in the place of curL (the bar counts roundings per visible key and per 32-key tile of
the logical sequence; a hidden key contributes to neither).

THE DECK.  H = 2, B2 <= 3, every (row, head) of a launch with its own mask.  `ends` is the kernel's argument, so the deck is free to cut the
cache as the coverage needs:
  * the pyramid (1, 2, 3, 4, 6), ends (1, 5, 14, 30, 66), with the query scales l = 1, 4, 9, 36 (36: a second wave with 4 queries);
  * two six-scale cuts of the same 66 keys, ends (1, 5, 14, 30, 61, 66) and (1, 5, 14, 30, 63, 66), whose fifth scale alone, or with the first,
    gives n = 31, 32, 33 (and 34): a last tile one short of full, full, and one and two keys into a second tile;
  * segments begin at the physical keys 1, 5, 14, 30: none a multiple of 4, and the one at 30 straddles the 32-key tile boundary (and, in
    logical positions, a different one per mask);
  * a hidden scale in the middle, the first scale hidden, the own (last) scale hidden, one scale alone (n = 1 among them), full masks (n = curL),
    n = 0 (an empty mask, and a mask whose only bits lie at or above S1), bits at or above S1 set beside a real mask (the sign bit included);
  * one case at l = 256 over the 680 keys of the pyramid (1, 2, 3, 4, 5, 6, 8, 10, 13, 16): two workgroups of four waves, 22 tiles.
Hidden scales, and the rows [curL, Lmax) of the cache, hold NaN in K and V; `out` starts as a sentinel.  COVERAGE states the above in numbers and
the CPU test recomputes it from the cases."""
import numpy as np

from tests.attncases import C_ROUND, E_EXP

SENTINEL = np.float32(-7.25)
PYR = (1, 5, 14, 30, 66)
CUT_A = (1, 5, 14, 30, 61, 66)
CUT_B = (1, 5, 14, 30, 63, 66)
BIG = (1, 5, 14, 30, 55, 91, 155, 255, 424, 680)
HI = -(1 << 31)                                   # the sign bit: a bit at or above S1


def cases():
    def c(name, ends, l, masks, pad=3):
        return dict(name=name, ends=tuple(ends), S1=len(ends), l=l, curL=ends[-1], Lmax=ends[-1] + pad, B2=len(masks), H=2, masks=[list(r) for r in masks])
    return [
        c('pyramid q0 l=1', PYR[:1], 1, [[1, 0], [1 | 2 | HI, 2 | 4]]),                                  # n = 1, 0, 1, 0 (only bits >= S1)
        c('pyramid q1 l=4', PYR[:2], 4, [[3, 1], [2, 3 | 4 | HI], [0, 2]]),                              # full, own hidden, first hidden, full, none, own only
        c('pyramid q2 l=9', PYR[:3], 9, [[7, 5], [6, 3], [4, 1]]),                                      # full, middle, first, own hidden, own only, n = 1
        c('pyramid q4 l=36', PYR, 36, [[31, 27], [30, 15], [16, 21]], pad=5),                           # ... own only begins at key 30; 21: every other scale
        c('cut A l=9', CUT_A, 9, [[16, 17], [63, 48], [16 | 64 | HI, 0]]),                              # n = 31, 32, 66, 36, 31, 0
        c('cut B l=4', CUT_B, 4, [[16, 17], [18, 63]], pad=1),                                          # n = 33, 34, 37, 66
        c('big l=256', BIG, 256, [[1023, 1023 & ~(1 << 8)], [1022, (1 << 9) | (1 << 3)]], pad=8),       # full, a middle scale, the first, two alone
    ]


def visible(ends, mask):
    """bool [curL]: key j belongs to a scale whose bit is set in mask (bits at or above len(ends) are ignored)"""
    vis = np.zeros(ends[-1], bool)
    b = 0
    for i, e in enumerate(ends):
        if (int(mask) >> i) & 1:
            vis[b:e] = True
        b = e
    return vis


def n_visible(c, b, h):
    return int(visible(c['ends'], c['masks'][b][h]).sum())


COVERAGE = dict(n=[0, 1, 31, 32, 33, 34], full=[1, 5, 14, 66, 680], l=[1, 4, 9, 36, 256], seg_begin_mod4=[1, 2, 3], straddle=True,
                first_hidden=True, middle_hidden=True, own_hidden=True, high_bits=True)


def coverage(cs=None):
    cs = cases() if cs is None else cs
    ns, full, begins = set(), set(), set()
    first = middle = own = high = straddle = False
    for c in cs:
        for b in range(c['B2']):
            for h in range(c['H']):
                m, S1, ends = c['masks'][b][h], c['S1'], c['ends']
                low = m & ((1 << S1) - 1)
                n = n_visible(c, b, h)
                ns.add(n)
                if low == (1 << S1) - 1:
                    full.add(n)
                high |= (m >> S1) != 0
                shown = [i for i in range(S1) if (low >> i) & 1]
                if shown:
                    first |= 0 not in shown and S1 > 1
                    own |= S1 - 1 not in shown
                    middle |= any(i not in shown for i in range(shown[0] + 1, shown[-1]))
                for i in shown:
                    pb = ends[i - 1] if i else 0
                    begins.add(pb % 4)
                    straddle |= pb % 32 != 0 and pb // 32 != (ends[i] - 1) // 32
    return dict(n=sorted(x for x in ns if x in COVERAGE['n']), full=sorted(full), l=sorted({c['l'] for c in cs}),
                seg_begin_mod4=sorted(begins - {0}), straddle=straddle, first_hidden=first, middle_hidden=middle, own_hidden=own, high_bits=high)


class Built:
    pass


_BUILT = {}


def build(c):
    """-> q [B2 l][H 64], k, v [B2][H][Lmax][64] float32, masks int32 [B2 H] (with the case's bits at or above S1 left as given), ends int32 [S1];
    K and V hold NaN in every hidden scale of their (row, head) and from curL on.  Computed once per case, shared and left unchanged."""
    if c['name'] in _BUILT:
        return _BUILT[c['name']]
    B2, H, l, curL, Lmax = c['B2'], c['H'], c['l'], c['curL'], c['Lmax']
    rng = np.random.default_rng(4100 + 7 * l + curL + len(c['name']))
    b = Built()
    b.case = c
    b.q = (0.45 * rng.standard_normal((B2, l, H, 64))).astype(np.float32).reshape(B2 * l, H * 64)
    b.k = np.full((B2, H, Lmax, 64), np.nan, np.float32)
    b.v = np.full((B2, H, Lmax, 64), np.nan, np.float32)
    for bb in range(B2):
        for h in range(H):
            vis = visible(c['ends'], c['masks'][bb][h])
            b.k[bb, h, :curL][vis] = (0.45 * rng.standard_normal((int(vis.sum()), 64))).astype(np.float32)
            b.v[bb, h, :curL][vis] = rng.standard_normal((int(vis.sum()), 64)).astype(np.float32)
    b.masks = np.array(c['masks'], dtype=np.int64).astype(np.int32).reshape(B2 * H)
    b.ends = np.array(c['ends'], dtype=np.int32)
    _BUILT[c['name']] = b
    return b


def q_of(b, bb, h):
    """the l queries of (row, head) as a contiguous [l][64] float32 array"""
    l = b.case['l']
    return np.ascontiguousarray(b.q[bb * l:(bb + 1) * l, h * 64:(h + 1) * 64])


def gather(mask, ends, k, v, shift=0):
    """k, v [Lmax][64] of one (row, head) -> (kc, vc [max(n, 1)][64], n): the rows of the visible scales, ascending, at 0 .. n - 1.
    shift (the CPU test's planted mistake): every visible scale but the first of the cache is taken `shift` rows further on."""
    rows, b = [], 0
    for i, e in enumerate(ends):
        if (int(mask) >> i) & 1:
            s = shift if b else 0
            rows.extend(range(b + s, e + s))
        b = e
    n = len(rows)
    kc, vc = np.full((max(n, 1), 64), np.nan, np.float32), np.full((max(n, 1), 64), np.nan, np.float32)
    kc[:n], vc[:n] = k[rows], v[rows]
    return kc, vc, n


def masked_reference(q, k, v, vis):
    """q [l][64], k, v [>= curL][64] float32 and the boolean key mask vis [curL] -> (ref, bar) [l][64] float64: softmax(q k^T) v over the visible
    keys of the ungathered cache, and the bar of tests/attncases.py for a cache of n = vis.sum() keys walked in 32-key tiles of the logical
    sequence (zeros and a zero bar for n = 0)"""
    l, n = q.shape[0], int(vis.sum())
    if n == 0:
        return np.zeros((l, 64)), np.zeros((l, 64))
    curL = len(vis)
    q, k, v = q.astype(np.float64), k[:curL].astype(np.float64), v[:curL].astype(np.float64)
    s = np.where(vis[None, :], q @ np.where(vis[:, None], k, 0.0).T, -np.inf)
    d = np.where(vis[None, :], s.max(1, keepdims=True) - s, 0.0)
    p = np.where(vis[None, :], np.exp(-d), 0.0)
    S = p.sum(1, keepdims=True)
    v0 = np.where(vis[:, None], v, 0.0)
    av = np.abs(v0)
    ref, pv = p @ v0 / S, p @ av
    aref = np.abs(ref)
    Ax = np.maximum(np.abs(q) @ np.abs(np.where(vis[:, None], k, 0.0)).T - 1.0, 0.0)
    logical = np.cumsum(vis) - 1                                                    # a visible key's position in the logical sequence
    R = np.where(vis, (n + 31) // 32 - 1 - logical // 32, 0).astype(np.float64)[None, :]
    eta = E_EXP * (1.0 + R) + 2.0 ** -24 * (R + d)
    bar = ((n + C_ROUND) * 2.0 ** -23 * pv / S
           + 64 * 2.0 ** -24 * ((p * Ax) @ av + aref * (p * Ax).sum(1, keepdims=True)) / S
           + ((p * eta) @ av + aref * (p * eta).sum(1, keepdims=True)) / S
           + n * 2.0 ** -125 * (av.max() + aref) / S)
    return ref, bar
