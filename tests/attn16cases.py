"""Two decks for the 16-bit attention kernel (var_amd/csrc/attn16.hip: varhip_attn_cached_f16 / _bf16), their operand builders, the float64
reference and its bar, shared by tests/test_attn16_dispatch_cpu.py (the decks proven on the CPU: conditions, coverage, the oracle's twins,
mutants of the reference) and tests/test_attn16_dispatch_gpu.py (the kernel itself, both flavours, every operand in a guard arena).
Rows [curL, Lmax) of K and V are NaN in every case of both decks: the kernel clamps the key index of its tile loads to curL - 1, and a
row read past that poisons the result.

THE SELECTOR DECK (sel_cases): exact, no tolerance.  Hd is the 64 x 64 Sylvester Hadamard matrix / 8: entries +-1/8, rows orthonormal.  In
a (b, h) slice every key is Hd[0] except a window of n <= 63 consecutive keys from key w on, which holds Hd[1 .. n]; query t is
128 Hd[1 + (a t + c) mod n] (entries +-16).  Every product of the score is +-2, every partial sum an integer of at most 128: the fp32 score
is exactly 128 for key sel(t) = w + (a t + c) mod n and exactly 0 for every other key, whatever the order of the sum.  In units of log2
the margin is 128 log2(e) = 184.66 > 150: every other p is exp2(below -150) = 0 in fp32, and whatever the accumulators held before the
selected key's tile is multiplied by alpha = exp2(-184.66) = 0.  p* = exp2(fma(128, log2e, -fl(128 log2e))) is 1 within an fp32 ulp of the
exponential and rounds to 1 in 16 bits; V holds integers of [-128, 128] (exact in both types, at most 8 significant bits), so O = v exactly,
the row sum is p*, and v / p* = v (1 +- 2^-22) rounds back to v: out[b, t, h, :] = v[b, h, sel(t), :] bit for bit in both flavours.  A wrong key
order between p and V^T in any register position, stage or tile, a wrong head, batch or Lmax stride returns another row; the rows of a slice
are pairwise distinct and differ from the same key's row of every other slice (asserted on the CPU).  SEL_COVERAGE states what the deck
covers; the CPU test recomputes every item from the cases.

The wave count.  attn16_waves(l) starts from NW = 4 and takes a smaller NW only for strictly fewer idle waves; NW = 1 leaves none, so the
choice is the largest NW of 4, 3, 2, 1 that divides nq = ceil(l / 32) (waves, restated here; the GPU test asserts varhip_attn16_last_waves()
against it case by case).  A consequence: no launch of this dispatch has a wave with t0 >= l — `if (t0 < l)` in the kernel is never false
for a whole wave, idle_waves() is 0 for every l (asserted for l up to 4096), and a case with an idle last wave cannot be built without a
hook that forces NW.  What can be built is: every NW with grid.x > 1, and a last wave that is partly idle (l % 32 != 0) under every NW.

THE BAR DECK (bar_cases): float64 reference, derived bar.  q, k, v are generated in float64 and rounded once to the 16-bit type; the reference
is softmax(q k^T) v in float64 numpy on the rounded values (key by key, no tiles, no oracle).  Scores are built, not drawn:
    k_j = g(j) / 8 Hd[0] + Hd[1 + j % 32] + Hd[33 + j // 32],   q_t = 8 Hd[0] + sum_p D[t, p] Hd[1 + p] + sum_kt E[t, kt] Hd[33 + kt]
give q_t . k_j = g(j) + D[t, j % 32] + E[t, j // 32] (plus a seeded perturbation of 2e-3 per element, so that the roundings are real).
D orders the 32 positions of a tile by rank(t, p) = (7 p + 11 t + off) % 32, a permutation of the positions for every query and of the
queries of a wave for every position, with `off` such that a chosen query ranks the LAST valid key first (its weight is what the key-count
mutants move).  The profiles (`kind`):
    asc     g = 3 kt: the tile maximum rises by 3 in every tile, the ragged one included (E lifts it by what its best valid position lacks)
    desc    g = -0.3 kt: the maximum stands in tile 0, no tile after the first rescales
    late    flat scores (spread 1.55) and +6 on the last valid key: one rescale, in the ragged tile
    split   desc, and E = +4 over tile 0 in tile `X` for the queries with t % 32 >= 16 only: __any is true with alpha = 1 in half the lanes
    split1  desc, and the same bump in the ragged tile for the one query t % 32 == 7 of every wave
    wide    D spans +-60 (the no-l2-norm mode's range), E moves the tile maximum by 2.5 per step in a query-dependent tile order
D = -0.7 min(rank, 8) outside `late` and `wide`: about two keys per tile carry the weight, the effective support 1 / sum (p / S)^2 stays below
16 keys (asserted), so that a misplaced key moves the output by far more than a bf16 rounding.

The bar, per output element, with u = 2^-11 (f16) / 2^-8 (bf16), d = 2^-25 (f16) / 0 (bf16), p_j = exp(s_j - max s), S = sum p_j, P|V| = sum p_j |v_j|:
    bar = [u P|V| + d sum_j |v_j|] / S  +  u |ref| + d  +  (curL + 72) 2^-23 P|V| / S  +  64 2^-24 [sum_j p_j A'_j |v_j| + |ref| sum_j p_j A'_j] / S
  * u P|V| / S: p is rounded to 16 bits for the second product only (the row sum adds the fp32 p), at p' = exp2(s - m_tile) >= p; the later
    rescales by alpha <= 1 keep the relative error.
  * d sum |v_j| / S: a p' below 2^-14 is an fp16 subnormal, spacing 2^-24, so its rounding is absolute, at most 2^-25, and alpha <= 1 only shrinks it.
  * u |ref| + d: the output's own rounding (+ d: an fp16 output below 2^-14; ADDED to the issue's formula, it is at most 3e-8).
  * (curL + 72) 2^-23 P|V| / S: fp32 everywhere else, first order.  The row sum and the p.v accumulation each pass a term through at most curL
    additions (curL 2^-24 each, on the numerator and on the denominator: together curL 2^-23); 72 = 64 for the additions of a score whose
    products sum to at most 1 in magnitude, and 8 for exp2, the fma into units of log2, the rounded log2(e), the rescales a term with weight
    left passes through, 1 / S and the final product.
  * the last term is ADDED to the issue's formula.  The score's 64 additions round at the magnitude of its partial sums, up to
    A_j = sum_d |q_d| |k_jd|, not at the magnitude of s_j; an absolute error e of s_j is a relative error e of p_j, in the numerator
    (p_j e |v_j|) and in the denominator (|ref| p_j e).  The 64 of the term above pays for A_j <= 1; A'_j = max(A_j - 1, 0) is the rest.  Its
    share of the bar (a property of the deck, computed from the formula): 8 to 22 % in f16 and 1 to 4 % in bf16 outside `wide`, 60 % in
    f16 and 16 % in bf16 on `wide`, where A_j is a few hundred.
Nothing here is measured.  Mutants of the reference that the CPU test holds against 2 bar: one key too many (key curL - 1 twice) / too few; the
O rescale, or the row-sum rescale, left out in the last tile where the query's running maximum moves; V rows j <-> j ^ 4, j <-> j ^ 16 swapped
inside the tile of the query's peak.  `sibling` names the case that stands in where a profile has no rescale after tile 0 (desc).
"""
import numpy as np

FLAVOURS = ('f16', 'bf16')
U16 = {'f16': 2.0 ** -11, 'bf16': 2.0 ** -8}
D16 = {'f16': 2.0 ** -25, 'bf16': 0.0}
TWIN = {'f16': 'attn_cached_p16_f32', 'bf16': 'attn_cached_pbf16_f32'}
LOG2E = 1.4426950408889634


def hadamard64():
    h = np.ones((1, 1))
    while h.shape[0] < 64:
        h = np.block([[h, h], [h, -h]])
    return h / 8.0


HD = hadamard64()


def round16(a, flav):
    """float64 -> the nearest value of the 16-bit type (ties to even), returned as float32 (exact: both types embed in fp32)"""
    a = np.asarray(a, np.float64)
    if flav == 'f16':
        return a.astype(np.float16).astype(np.float32)
    m, e = np.frexp(a)                                    # |m| in [0.5, 1): 8 significant bits = multiples of 2^-8 (fp32's exponent range: no subnormals met here)
    return np.ldexp(np.round(m * 256.0) / 256.0, e).astype(np.float32)


class Built:
    pass


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch, restated
def waves(l):
    nq = (l + 31) // 32
    best, waste = 4, (nq + 3) // 4 * 4 - nq
    for nw in (3, 2, 1):
        w = (nq + nw - 1) // nw * nw - nq
        if w < waste:
            best, waste = nw, w
    return best


def grid_x(l):
    return (l + waves(l) * 32 - 1) // (waves(l) * 32)


def idle_waves(l):
    """waves of the launch whose first query t0 is >= l"""
    return grid_x(l) * waves(l) - (l + 31) // 32


# ---------------------------------------------------------------------------------------------------------------------
# the selector deck
def sel_cases():
    def c(l, curL, pad, B2, H):
        return dict(name=f'sel l={l} curL={curL} Lmax={curL + pad} B2={B2} H={H}', l=l, curL=curL, Lmax=curL + pad, B2=B2, H=H, nw=waves(l))
    return [c(1, 1, 39, 1, 1),             # the first scale: one query, one key
            c(16, 30, 0, 1, 2),            # a single, ragged tile; the cache ends with the last key
            c(31, 37, 33, 2, 3),           # curL % 32 = 5, two tiles
            c(33, 81, 0, 2, 1),            # 17, three tiles; NW = 2 with one query in the second wave
            c(64, 95, 40, 1, 3),           # 31, three tiles
            c(65, 97, 33, 2, 3),           # 1, four tiles; NW = 3
            c(96, 160, 0, 2, 3),           # no ragged tile, five tiles
            c(97, 129, 35, 1, 2),          # 1, five tiles; NW = 4
            c(128, 192, 64, 2, 3),         # no ragged tile, six tiles: every key of every position and stage is selected
            c(130, 197, 0, 1, 3),          # 5, seven tiles; NW = 1, grid.x = 5
            c(161, 241, 33, 2, 3),         # 17, eight tiles; NW = 3, grid.x = 2
            c(250, 273, 0, 1, 2),          # 17, nine tiles; NW = 4, grid.x = 2
            c(300, 319, 33, 2, 1)]         # 31, ten tiles; NW = 2, grid.x = 5


_STEPS = (1, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)


def sel_windows(c):
    """-> [(w, n, a, c0)] per slice i = b H + h: window start and length, sel(t) = w + (a t + c0) % n with gcd(a, n) = 1.  Slice 0's window ends
    with the last key, slice 1's starts at key 0, the others lie evenly between; n = min(63, l, curL), so every window key is selected"""
    S = c['B2'] * c['H']
    n = min(63, c['l'], c['curL'])
    out = []
    for i in range(S):
        w = (c['curL'] - n) * ((i - 1) % S) // max(S - 1, 1) if S > 1 else c['curL'] - n
        a = next(s for s in _STEPS[i:] + _STEPS if np.gcd(s, n) == 1)
        out.append((w, n, a, 4 * i + 4))
    return out


def sel_keys(c):
    """-> int [B2][H][l]: the key each query selects"""
    t = np.arange(c['l'])
    return np.stack([w + (a * t + c0) % n for w, n, a, c0 in sel_windows(c)]).reshape(c['B2'], c['H'], c['l'])


def build_selector(c):
    """-> q [B2 l][H 64], k, v [B2][H][Lmax][64] float32 (exact in f16 and bf16; NaN rows from curL on), sel, expected [B2 l][H 64]"""
    B2, H, l, curL, Lmax = c['B2'], c['H'], c['l'], c['curL'], c['Lmax']
    rng = np.random.default_rng(7000 + 1000 * l + curL)
    b = Built()
    b.case, b.sel = c, sel_keys(c)
    b.k = np.full((B2, H, Lmax, 64), np.nan, np.float32)
    b.v = np.full((B2, H, Lmax, 64), np.nan, np.float32)
    b.k[:, :, :curL] = HD[0]
    b.v[:, :, :curL] = rng.integers(-128, 129, (B2, H, curL, 64))
    b.q = np.empty((B2, l, H, 64), np.float32)
    t = np.arange(l)
    for i, (w, n, a, c0) in enumerate(sel_windows(c)):
        bb, h = divmod(i, H)
        b.k[bb, h, w:w + n] = HD[1:1 + n]
        b.q[bb, :, h] = 128.0 * HD[1 + (a * t + c0) % n]
    b.expected = np.stack([b.v[bb, h, b.sel[bb, h]] for bb in range(B2) for h in range(H)]).reshape(B2, H, l, 64).transpose(0, 2, 1, 3)
    b.q, b.expected = b.q.reshape(B2 * l, H * 64), np.ascontiguousarray(b.expected).reshape(B2 * l, H * 64)
    return b


def sel_coverage(cases=None):
    """what the deck's selected keys cover, computed from the cases (SEL_COVERAGE below states the same as data)"""
    cases = sel_cases() if cases is None else cases
    stage_pos, lane_half, ragged, lane_pos = set(), set(), {}, set()
    for c in cases:
        sel = sel_keys(c).reshape(-1, c['l'])
        ntile, r = (c['curL'] + 31) // 32, c['curL'] % 32
        t = np.broadcast_to(np.arange(c['l']), sel.shape)
        full = sel // 32 < c['curL'] // 32                               # keys of whole tiles
        stage_pos |= set(zip(((sel // 32) & 1)[full].tolist(), (sel % 32)[full].tolist()))
        lane_half |= set(zip((t % 32).reshape(-1).tolist(), ((sel >> 2) & 1).reshape(-1).tolist()))
        lane_pos |= set(zip((t % 32).reshape(-1).tolist(), (sel % 32).reshape(-1).tolist()))
        if r:
            ragged.setdefault(r, set())
            ragged[r] |= set((sel % 32)[sel // 32 == ntile - 1].tolist())
    return dict(
        stage_pos=len(stage_pos),                                          # (stage = tile & 1, position in the tile) pairs selected in whole tiles
        ragged_complete=sorted(r for r, s in ragged.items() if s == set(range(r))),      # curL % 32 whose ragged tile has every valid position selected
        exact_multiple=[c['name'] for c in cases if c['curL'] % 32 == 0],
        single_tile=[c['name'] for c in cases if c['curL'] <= 32],
        ntile_parity=sorted({((c['curL'] + 31) // 32) & 1 for c in cases}),
        ragged_last_stage=sorted({(c['curL'] % 32, ((c['curL'] + 31) // 32 - 1) & 1) for c in cases if c['curL'] % 32 in (1, 5, 17, 31)}),
        lane_half=len(lane_half),                                          # (query lane t % 32, lane half (key >> 2) & 1 that holds the selected key's register)
        lane_pos=len(lane_pos),                                            # (query lane, key position) pairs, of 1024
        nw={nw: sorted(c['l'] for c in cases if c['nw'] == nw) for nw in (1, 2, 3, 4)},
        nw_grid_gt1=sorted({c['nw'] for c in cases if grid_x(c['l']) > 1}),
        nw_partial_last_wave=sorted({c['nw'] for c in cases if c['l'] % 32}),
        idle_waves=sorted({idle_waves(c['l']) for c in cases}),
        b2_h=sorted({(c['B2'], c['H']) for c in cases}),
        lmax_pad33=sum(c['Lmax'] >= c['curL'] + 33 for c in cases),
        cases=len(cases))


SEL_COVERAGE = dict(
    stage_pos=64, ragged_complete=[1, 5, 17, 30, 31],
    exact_multiple=['sel l=96 curL=160 Lmax=160 B2=2 H=3', 'sel l=128 curL=192 Lmax=256 B2=2 H=3'],
    single_tile=['sel l=1 curL=1 Lmax=40 B2=1 H=1', 'sel l=16 curL=30 Lmax=30 B2=1 H=2'],
    ntile_parity=[0, 1],
    ragged_last_stage=[(1, 0), (1, 1), (5, 0), (5, 1), (17, 0), (17, 1), (31, 0), (31, 1)],
    lane_half=64, lane_pos=1002,
    nw={1: [1, 16, 31, 130], 2: [33, 64, 300], 3: [65, 96, 161], 4: [97, 128, 250]},
    nw_grid_gt1=[1, 2, 3, 4], nw_partial_last_wave=[1, 2, 3, 4], idle_waves=[0],
    b2_h=[(1, 1), (1, 2), (1, 3), (2, 1), (2, 3)], lmax_pad33=8, cases=13)


# ---------------------------------------------------------------------------------------------------------------------
# the bar deck
def bar_cases():
    def c(kind, l, curL, pad, B2, H, sibling=None, X=None):
        return dict(name=f'{kind} l={l} curL={curL} Lmax={curL + pad} B2={B2} H={H}', kind=kind, l=l, curL=curL, Lmax=curL + pad, B2=B2, H=H,
                    nw=waves(l), sibling=sibling, X=X)
    asc = c('asc', 97, 145, 33, 2, 2)
    return [asc,
            c('asc', 33, 85, 0, 1, 3),
            c('desc', 65, 127, 40, 2, 1, sibling=asc['name']),
            c('desc', 130, 160, 0, 1, 2, sibling=asc['name']),
            c('late', 64, 95, 33, 1, 3),
            c('split', 96, 177, 0, 2, 2, X=3),
            c('split1', 40, 113, 35, 1, 2, X=3),
            c('wide', 128, 200, 56, 1, 2),
            c('wide', 31, 63, 0, 2, 1)]


T_PICK = {'asc': 3, 'desc': 3, 'late': 3, 'split': 3, 'split1': 3, 'wide': 2}      # wide: t = 2 (mod ntile) has its largest E in the last tile


def score_parts(c, i):
    """-> g [curL], D [l][32], E [l][ntile] of slice i: the score of (t, j) is built as g[j] + D[t, j % 32] + E[t, j // 32]"""
    l, curL, kind = c['l'], c['curL'], c['kind']
    ntile, j, t = (curL + 31) // 32, np.arange(curL), np.arange(l)[:, None]
    kt, last = j // 32, ntile - 1
    pick = T_PICK[kind] + ntile * i
    pick = pick if pick < l else T_PICK[kind]
    off = -(7 * ((curL - 1) % 32) + 11 * pick) % 32
    rank = (7 * np.arange(32)[None, :] + 11 * t + off) % 32
    g, D, E = np.zeros(curL), -0.7 * np.minimum(rank, 8), np.zeros((l, ntile))
    if kind == 'asc':
        g = 3.0 * kt
        E[:, last] = 0.7 * np.minimum(rank[:, :(curL - 1) % 32 + 1].min(1), 8)         # the ragged tile's best valid position is lifted to rank 0
    elif kind in ('desc', 'split', 'split1'):
        g = -0.3 * kt
        if kind == 'split':
            E[(t[:, 0] % 32) >= 16, c['X']] = 0.3 * c['X'] + 4.0
        if kind == 'split1':
            E[(t[:, 0] % 32) == 7, last] = 0.3 * last + 4.0
    elif kind == 'late':
        D = -0.05 * rank
        g[curL - 1] = 6.0
    elif kind == 'wide':
        D = 60.0 - (120.0 / 31.0) * rank
        E = 2.5 * ((3 * np.arange(ntile)[None, :] + t) % ntile)
    return g, D.astype(np.float64), E


def build_bar(c, flav):
    """-> q [B2 l][H 64], k, v [B2][H][Lmax][64] float32 holding values of the 16-bit type (NaN rows from curL on)"""
    B2, H, l, curL, Lmax = c['B2'], c['H'], c['l'], c['curL'], c['Lmax']
    ntile = (curL + 31) // 32
    b = Built()
    b.case, b.flav = c, flav
    b.k = np.full((B2, H, Lmax, 64), np.nan, np.float32)
    b.v = np.full((B2, H, Lmax, 64), np.nan, np.float32)
    b.q = np.empty((B2, l, H, 64), np.float32)
    j = np.arange(curL)
    for i in range(B2 * H):
        bb, h = divmod(i, H)
        rng = np.random.default_rng(9000 + 100 * l + curL + 7 * i)              # (no flavour: both round the same float64 values)
        g, D, E = score_parts(c, i)
        k = (g / 8.0)[:, None] * HD[0] + HD[1 + j % 32] + HD[33 + j // 32] + 2e-3 * rng.standard_normal((curL, 64))
        q = 8.0 * HD[0] + D @ HD[1:33] + E @ HD[33:33 + ntile] + 2e-3 * rng.standard_normal((l, 64))
        b.k[bb, h, :curL], b.q[bb, :, h] = round16(k, flav), round16(q, flav)
        b.v[bb, h, :curL] = round16(rng.standard_normal((curL, 64)), flav)
    b.q = b.q.reshape(B2 * l, H * 64)
    return b


def slices(b):
    """(b, h, q [l][64], k [curL][64], v [curL][64]) in float64, slice by slice"""
    c = b.case
    q = b.q.reshape(c['B2'], c['l'], c['H'], 64)
    for bb in range(c['B2']):
        for h in range(c['H']):
            yield bb, h, q[bb, :, h].astype(np.float64), b.k[bb, h, :c['curL']].astype(np.float64), b.v[bb, h, :c['curL']].astype(np.float64)


def _place(c, per_slice):
    """[(b, h, [l][64])] -> [B2 l][H 64]"""
    out = np.empty((c['B2'], c['l'], c['H'], 64))
    for bb, h, o in per_slice:
        out[bb, :, h] = o
    return out.reshape(c['B2'] * c['l'], c['H'] * 64)


def reference(b):
    """-> (ref, bar) [B2 l][H 64] float64 (module docstring); also b.support = the largest effective support 1 / sum (p / S)^2 of a query"""
    c, u, d = b.case, U16[b.flav], D16[b.flav]
    refs, bars, support = [], [], 0.0
    for bb, h, q, k, v in slices(b):
        s = q @ k.T
        p = np.exp(s - s.max(1, keepdims=True))
        S = p.sum(1, keepdims=True)
        ref, pv = p @ v / S, p @ np.abs(v)
        Ax = np.maximum(np.abs(q) @ np.abs(k).T - 1.0, 0.0)
        bar = ((u * pv + d * np.abs(v).sum(0)[None, :]) / S + u * np.abs(ref) + d + (c['curL'] + 72) * 2.0 ** -23 * pv / S
               + 64 * 2.0 ** -24 * ((p * Ax) @ np.abs(v) + np.abs(ref) * (p * Ax).sum(1, keepdims=True)) / S)
        refs.append((bb, h, ref)); bars.append((bb, h, bar))
        support = max(support, float((1.0 / ((p / S) ** 2).sum(1)).max()))
    b.support = support
    return _place(c, refs), _place(c, bars)


def tile_walk(s):
    """scores [l][curL] -> (running maximum after every tile [l][ntile], the last tile in which it moved [l] (0: it stands from tile 0 on),
    the tile of the peak [l])"""
    ntile = (s.shape[1] + 31) // 32
    tmax = np.stack([s[:, kt * 32:kt * 32 + 32].max(1) for kt in range(ntile)], 1)
    run = np.maximum.accumulate(tmax, 1)
    moved = np.concatenate([np.ones((s.shape[0], 1), bool), run[:, 1:] > run[:, :-1]], 1)
    return run, ntile - 1 - np.argmax(moved[:, ::-1], 1), s.argmax(1) // 32


MUTANTS = ('one key more', 'one key less', 'no O rescale', 'no row-sum rescale', 'swap j^4', 'swap j^16')
NEED_MOVE = ('no O rescale', 'no row-sum rescale')


def mutant(b, what):
    """the float64 reference with one planted fault -> [B2 l][H 64]"""
    c = b.case
    outs = []
    for bb, h, q, k, v in slices(b):
        if what == 'one key more':
            k, v = np.concatenate([k, k[-1:]]), np.concatenate([v, v[-1:]])
        elif what == 'one key less':
            k, v = k[:-1], v[:-1]
        s = q @ k.T
        p = np.exp(s - s.max(1, keepdims=True))
        num, S = p @ v, p.sum(1, keepdims=True)
        if what in NEED_MOVE:
            run, kstar, _ = tile_walk(s)
            rows = np.arange(s.shape[0])
            # the tiles before kstar were accumulated relative to run[kstar - 1]; the fault leaves out alpha = exp(run[kstar - 1] - run[kstar])
            alpha = np.where(kstar > 0, np.exp(run[rows, np.maximum(kstar - 1, 0)] - run[rows, kstar]), 1.0)[:, None]
            before = np.arange(s.shape[1])[None, :] < (kstar * 32)[:, None]
            pb = np.where(before, p, 0.0)
            if what == 'no O rescale':
                num = num + (1.0 / alpha - 1.0) * (pb @ v)
            else:
                S = S + (1.0 / alpha - 1.0) * pb.sum(1, keepdims=True)
        elif what.startswith('swap'):
            x = int(what.split('^')[1])
            _, _, peak = tile_walk(s)
            for kt in np.unique(peak):
                js = np.arange(kt * 32, min(kt * 32 + 32, s.shape[1]))
                jx = np.where((js ^ x) < s.shape[1], js ^ x, js)
                rows = peak == kt
                num[rows] += p[rows][:, js] @ (v[jx] - v[js])
        outs.append((bb, h, num / S))
    return _place(c, outs)


def within(name, got, ref, bar):
    """assert |got - ref| <= bar elementwise; prints and returns max err / bar"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, f'{name}: shape {got.shape} != {ref.shape}'
    assert np.isfinite(got).all(), f'{name}: non-finite results at {tuple(np.argwhere(~np.isfinite(got))[0])} (a row past curL or a band was read?)'
    err = np.abs(got - ref)
    ratio = float((err / bar).max())
    print(f'{name}: max err / bar = {ratio:.4f}')
    bad = ~(err <= bar)
    assert not bad.any(), (f'{name}: {int(bad.sum())}/{bad.size} outside the float64 bar (max err / bar = {ratio:.3f}), first at '
                           f'{tuple(np.argwhere(bad)[0])}: got {got[tuple(np.argwhere(bad)[0])]!r} ref {ref[tuple(np.argwhere(bad)[0])]!r}')
    return ratio


def twin(L, flav, b):
    """the oracle's twin of the flavour on the case's float32 operands -> [B2 l][H 64] float32"""
    from oracle.var_oracle import _p
    c = b.case
    out = np.full((c['B2'] * c['l'], c['H'] * 64), np.nan, np.float32)
    q, k, v = (np.ascontiguousarray(a, dtype=np.float32) for a in (b.q, b.k, b.v))
    assert L[TWIN[flav]](_p(q), _p(k), _p(v), _p(out), c['B2'], c['l'], c['H'], c['curL'], c['Lmax']) == 0
    return out
