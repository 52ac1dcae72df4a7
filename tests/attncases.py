"""Three decks for the fp32 attention kernel (var_amd/csrc/attn.hip: varhip_attn_cached_f32), their operand builders, the float64 reference and
its bar, shared by tests/test_attn_dispatch_cpu.py (the decks proven on the CPU: conditions, coverage, the oracle's twin, mutants of the
reference) and tests/test_attn_dispatch_gpu.py (the kernel itself, every operand in a guard arena).  Built on tests/attn16cases.py: the Hadamard
matrix, the restated dispatch (the fp32 launcher's attn_waves is the 16-bit one's rule), the selector windows, the score profiles, the tile walk
and the mutants of the reference are type-independent and imported from there.  Rows [curL, Lmax) of K and V are NaN in every case of every
deck: the kernel clamps the key index of its tile loads to curL - 1, and a row read past that poisons the result.

THE SELECTOR DECK (sel_cases, the 16-bit deck's list): exact, no tolerance.  Keys are rows of Hd (64 x 64 Sylvester Hadamard / 8) and query t is
128 Hd[1 + ...], as in the 16-bit deck: every product of the score is +-2 and every partial sum an integer of at most 128, so the fp32 score is
exactly 128 for key sel(t) and exactly 0 for every other key in ANY order of the sum (asserted for two orders).  What differs from the 16-bit
kernel: vm_exp_le0 (include/var_math.h) clamps its argument at -87 and never returns 0.  With eps = vm_exp_le0(-87) = 1.65e-38 < 2^-125:
  * before the selected key's tile the maximum is 0, every p is vm_exp_le0(0) = 1.0 exactly, and the accumulators hold exact integers (sums of at
    most 319 values of at most 128); in that tile alpha = vm_exp_le0(0 - 128) = eps, NOT 0: what the accumulators held survives as a stray term of
    at most curL 128 eps, and every non-selected key of that and of every later tile adds p v = eps v, at most 128 eps, not 0;
  * p* = vm_exp_le0(128 - 128) = 1.0 exactly; the stray mass of an accumulator is at most curL 128 2^-125 <= 2^-109 in all, far below half an ulp
    (2^-24) of a value of magnitude >= 1.  So IF v* != 0 the fma that adds 1.0 v* rounds to v*, every later fma(eps, v, v*) rounds back to v*, and
    later tiles rescale by vm_exp_le0(0) = 1.0.  With v* = 0 the accumulator would keep the stray term and the result would be 1e-36, not 0:
    V therefore holds NON-ZERO integers of [-128, 128];
  * the partial row sum that receives p* is 1.0 + stray = 1.0, the other three are stray, (S00 + S01) + (S10 + S11) rounds to 1.0, inv = 1.0,
    out = v* 1.0:   out[b, t, h, :] == v[b, h, sel(t), :]   bit for bit.
(Subnormal products, whether kept or flushed, only change the stray term.)  The argument is proven on the CPU: varref_attn_cached_f32 returns
exactly the selected rows on every case.  A wrong key order between p and V^T in any register position, stage or tile, a wrong head, batch or
Lmax stride returns another row; the rows of a slice are pairwise distinct and differ from the same key's row of every other slice (asserted).
SEL_COVERAGE states what the deck covers (all 32 positions of a tile in both K stages kt & 1, the ragged tile's last valid key, every NW with
grid.x > 1 and with a partly idle last wave); the CPU test recomputes every item from the cases.

THE BAR DECK (bar_cases, the 16-bit deck's list and score profiles asc / desc / late / split / split1 / wide: attn16cases.py says what each does
to the running maximum): float64 reference, derived bar.  q, k, v are generated in float64 and rounded once to fp32; the reference is
softmax(q k^T) v in float64 numpy on the rounded values (key by key, no tiles, no oracle).  The effective support 1 / sum (p / S)^2 stays below
16 keys (asserted), so that a misplaced key moves the output by far more than the bar.

The bar, per output element.  With d_j = max s - s_j, p_j = exp(-d_j), S = sum p_j (>= 1), P|V| = sum p_j |v_j|, A_j = sum_d |q_d| |k_jd|,
A'_j = max(A_j - 1, 0), ntile = ceil(curL / 32), R_j = ntile - 1 - j // 32 (the tiles after key j's: the rescales its weight can pass through):
    bar = (curL + 66) 2^-23 P|V| / S
        + 64 2^-24 [sum_j p_j A'_j |v_j| + |ref| sum_j p_j A'_j] / S
        + [sum_j p_j eta_j |v_j| + |ref| sum_j p_j eta_j] / S,      eta_j = E (1 + R_j) + 2^-24 (R_j + d_j),   E = 4e-7
        + curL 2^-125 (max|v| + |ref|) / S
First order in 2^-24, every rounding counted once on the numerator sum p v and once on the denominator S (a relative error e of the denominator
moves the output by e |ref|, and |ref| <= P|V| / S):
  * (curL + 66) 2^-23 P|V| / S.  curL: the p.v fma chain and the row sum each pass a term through at most curL roundings (curL 2^-24 on either side,
    together curL 2^-23).  66 = 64 + 1 + 1: 64 for the 64 fmas of a score whose products sum to at most 1 in magnitude (an absolute error e of s_j
    is a relative error e of p_j, on both sides); 1 for inv = 1 / S and the product O inv (two roundings of the output, 2^-23 |ref|); 1 for what the
    first order leaves out (at most 512 factors (1 + 2^-24) multiply to 1 + 512 2^-24 (1 + 2^-15): the excess is below 2^-15 of the bar).
  * the A' term: the score's additions round at the magnitude of its partial sums, up to A_j, not at the magnitude of s_j.  The 64 above pays for
    A_j <= 1, this pays for the rest (`wide`: A_j is a few hundred).
  * the eta term: the relative error of vm_exp_le0, applied to the numerator and to the denominator.  E = 4e-7 is the bound the project asserts in
    test_vm_log_exp_accuracy (tests/test_oracle_vs_golden.py) for the shared polynomial; test_attn_dispatch_cpu.py holds vm_exp_le0 itself to it on
    [-87, 0] through the twin.  A key's final weight is p_j times every alpha = vm_exp_le0(m_old - m_new) of the later tiles: 1 + R_j exponentials at
    the most (alpha is exactly 1.0 where the maximum stands).  Their arguments are differences: s_j - m and m_old - m_new round with at most
    2^-24 of their magnitudes, which add up to d_j along the key's path (all of one sign); each rescale is one more multiply, 2^-24.  The issue's
    count puts the exponent's argument and the rescales into the constant; here they depend on the key, so they are counted per key instead.
    (R_j counts every later tile, moved maximum or not: no assumption about which tiles rescale.)
  * curL 2^-125 (max|v| + |ref|) / S, for the clamp: a weight whose path met the clamp at -87 is at most eps (1 + E) < 2^-125 where it should be
    smaller still, an absolute error below 2^-125 per key on either side (the |ref| half is ADDED to the issue's formula, for the denominator).
Nothing here is measured.  Mutants of the reference that the CPU test holds against 2 bar (attn16cases.mutant): one key too many (key curL - 1
twice) / too few; the O rescale, or the row-sum rescale, left out in the last tile where the query's running maximum moves; V rows j <-> j ^ 4,
j <-> j ^ 16 swapped inside the tile of the query's peak.  `sibling` names the case that stands in where a profile has no rescale after tile 0.

THE FORCED-NW DECK (forced_cases): l in {1, 33, 65, 97, 130} with a ragged curL and Lmax > curL, B2 = 2, H = 2, inputs of a bar-deck profile, each
launched under varhip_attn_force_waves(1 .. 4).  The dispatch's own choice never leaves a wave without queries (idle_waves(l) == 0 for every l);
a forced NW does: forced_idle(l, nw) waves of the launch have t0 >= l and only stage and sync (FORCED_IDLE states the table, the CPU test
recomputes it: 1, 2 and 3 idle waves each occur, and every NW >= 2 has a case with some).  A query's arithmetic depends on its own wave's 32
queries and on the tile walk, never on NW: the GPU test asserts bit-identity with the unforced launch, and the bar.
"""
import numpy as np

from tests import attn16cases as ac16
from tests.attn16cases import (HD, MUTANTS, NEED_MOVE, Built, grid_x, idle_waves, mutant, score_parts, sel_cases, sel_keys,      # noqa: F401
                               sel_windows, slices, tile_walk, waves, within)

E_EXP = 4e-7            # the relative error of the exponential: the bound asserted by test_vm_log_exp_accuracy (tests/test_oracle_vs_golden.py)
C_ROUND = 66            # module docstring: 64 + 1 + 1
TWIN = 'attn_cached_f32'

bar_cases = ac16.bar_cases


# ---------------------------------------------------------------------------------------------------------------------
# the selector deck
def build_selector(c):
    """the 16-bit deck's operands (keys, queries, windows) with V redrawn from the NON-ZERO integers of [-128, 128] (module docstring)
    -> q [B2 l][H 64], k, v [B2][H][Lmax][64] float32 (NaN rows from curL on), sel [B2][H][l], expected [B2 l][H 64]"""
    B2, H, l, curL = c['B2'], c['H'], c['l'], c['curL']
    b = ac16.build_selector(c)
    rng = np.random.default_rng(17000 + 1000 * l + curL)
    shape = (B2, H, curL, 64)
    b.v[:, :, :curL] = rng.integers(1, 129, shape) * rng.choice([-1, 1], shape)
    exp = np.stack([b.v[bb, h, b.sel[bb, h]] for bb in range(B2) for h in range(H)]).reshape(B2, H, l, 64).transpose(0, 2, 1, 3)
    b.expected = np.ascontiguousarray(exp).reshape(B2 * l, H * 64)
    return b


def sel_coverage(cases=None):
    """attn16cases.sel_coverage of the cases, and where the ragged tile's LAST valid key (curL - 1) is selected"""
    cases = sel_cases() if cases is None else cases
    cov = ac16.sel_coverage(cases)
    cov['last_key_selected'] = sorted({c['curL'] % 32 for c in cases if c['curL'] % 32 and (sel_keys(c) == c['curL'] - 1).any()})      # curL % 32 of such cases
    return cov


SEL_COVERAGE = dict(ac16.SEL_COVERAGE, last_key_selected=[1, 5, 17, 30, 31])


# ---------------------------------------------------------------------------------------------------------------------
# the bar deck
def build_bar(c):
    """-> q [B2 l][H 64], k, v [B2][H][Lmax][64] float32: the float64 operands of the case's score profile rounded once (NaN rows from curL on)"""
    B2, H, l, curL, Lmax = c['B2'], c['H'], c['l'], c['curL'], c['Lmax']
    ntile = (curL + 31) // 32
    b = Built()
    b.case = c
    b.k = np.full((B2, H, Lmax, 64), np.nan, np.float32)
    b.v = np.full((B2, H, Lmax, 64), np.nan, np.float32)
    b.q = np.empty((B2, l, H, 64), np.float32)
    j = np.arange(curL)
    for i in range(B2 * H):
        bb, h = divmod(i, H)
        rng = np.random.default_rng(29000 + 100 * l + curL + 7 * i)
        g, D, E = score_parts(c, i)
        k = (g / 8.0)[:, None] * HD[0] + HD[1 + j % 32] + HD[33 + j // 32] + 2e-3 * rng.standard_normal((curL, 64))
        q = 8.0 * HD[0] + D @ HD[1:33] + E @ HD[33:33 + ntile] + 2e-3 * rng.standard_normal((l, 64))
        b.k[bb, h, :curL], b.q[bb, :, h] = k.astype(np.float32), q.astype(np.float32)
        b.v[bb, h, :curL] = rng.standard_normal((curL, 64)).astype(np.float32)
    b.q = b.q.reshape(B2 * l, H * 64)
    return b


def reference(b):
    """-> (ref, bar) [B2 l][H 64] float64 (module docstring); also b.support = the largest effective support 1 / sum (p / S)^2 of a query"""
    c = b.case
    curL = c['curL']
    R = ((curL + 31) // 32 - 1 - np.arange(curL) // 32).astype(np.float64)[None, :]
    refs, bars, support = [], [], 0.0
    for bb, h, q, k, v in slices(b):
        s = q @ k.T
        d = s.max(1, keepdims=True) - s
        p = np.exp(-d)
        S = p.sum(1, keepdims=True)
        av = np.abs(v)
        ref, pv = p @ v / S, p @ av
        aref = np.abs(ref)
        Ax = np.maximum(np.abs(q) @ np.abs(k).T - 1.0, 0.0)
        eta = E_EXP * (1.0 + R) + 2.0 ** -24 * (R + d)
        bar = ((curL + C_ROUND) * 2.0 ** -23 * pv / S
               + 64 * 2.0 ** -24 * ((p * Ax) @ av + aref * (p * Ax).sum(1, keepdims=True)) / S
               + ((p * eta) @ av + aref * (p * eta).sum(1, keepdims=True)) / S
               + curL * 2.0 ** -125 * (av.max() + aref) / S)
        refs.append((bb, h, ref)); bars.append((bb, h, bar))
        support = max(support, float((1.0 / ((p / S) ** 2).sum(1)).max()))
    b.support = support
    return ac16._place(c, refs), ac16._place(c, bars)


_BUILT = {}


def bar_built(c):
    """(operands, ref, bar) of a bar or forced case, computed once per test run, shared by the tests and left unchanged"""
    if c['name'] not in _BUILT:
        b = build_bar(c)
        _BUILT[c['name']] = (b,) + reference(b)
    return _BUILT[c['name']]


def twin(L, b):
    """varref_attn_cached_f32 on the case's operands -> [B2 l][H 64] float32 (NaN where it wrote nothing)"""
    from oracle.var_oracle import _p
    c = b.case
    out = np.full((c['B2'] * c['l'], c['H'] * 64), np.nan, np.float32)
    q, k, v = (np.ascontiguousarray(a, dtype=np.float32) for a in (b.q, b.k, b.v))
    assert L[TWIN](_p(q), _p(k), _p(v), _p(out), c['B2'], c['l'], c['H'], c['curL'], c['Lmax']) == 0
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the forced-NW deck
def forced_cases():
    def c(kind, l, curL, pad, X=None):
        return dict(name=f'forced {kind} l={l} curL={curL} Lmax={curL + pad}', kind=kind, l=l, curL=curL, Lmax=curL + pad, B2=2, H=2,
                    nw=waves(l), sibling=None, X=X)
    return [c('asc', 1, 37, 33),
            c('late', 33, 81, 40),
            c('split1', 65, 113, 33),
            c('split', 97, 177, 35, X=3),
            c('wide', 130, 197, 33)]


def forced_idle(l, nw):
    """waves of a launch with NW = nw whose first query t0 is >= l"""
    nq = (l + 31) // 32
    return (nq + nw - 1) // nw * nw - nq


FORCED_IDLE = {1: [0, 1, 2, 3], 33: [0, 0, 1, 2], 65: [0, 1, 0, 1], 97: [0, 0, 2, 0], 130: [0, 1, 1, 3]}      # l -> idle waves under NW = 1, 2, 3, 4
