"""One case table, one operand builder and one float64 reference for varhip_gemm_nt_f32 / varhip_gemm_qkv_f32 (and their twins), shared by
tests/test_gemm_dispatch_cpu.py (the twins alone) and tests/test_gemm_dispatch_gpu.py (every dispatch path of var_amd/csrc/gemm.hip).

Operands.  Every operand is allocated with its own leading dimension, batch stride and element offset (an interior pointer is passed as
(array, element_offset), the form tests/test_kernels_gpu.py::both takes).  Real elements are seeded normals at the scales of test_gemm_exact
(A 1, W 0.05, bias 0.1, resid 1, gamma 1); EVERY other element of A, W, bias, resid and gamma — row padding, batch padding, the elements in
front of an interior pointer and a short tail — is NaN, so a stray read poisons the result.  The whole `out` allocation is filled with one
sentinel bit pattern (SENTINEL_BITS, a NaN with a payload).  After the call every element inside [M][N] of each batch must differ from the
sentinel and be finite, every other element must still hold it, bit for bit.

Reference and bound.  The reference is float64 numpy: x = A64 @ W64^T + bias, then the epilogue in float64 (gelu_tanh by the formula of
include/var_math.h, x / (1 + exp(-2u)), u = c0 (x + c1 x^3), with that header's fp32 constants).  With u = 2^-24 (the unit roundoff of fp32):

  * no epilogue.  The kernel computes one k-ascending fma chain from 0 and one add of the bias: K + 1 roundings, each a relative
    perturbation of at most u of a partial sum.  The standard forward bound of such a chain (Higham, Accuracy and Stability of Numerical
    Algorithms, section 3.1) is |got - x| <= gamma_{K+1} S with S = sum_k |a_k w_k| + |bias| and gamma_n = n u / (1 - n u); for the K of the
    table ((K + 1)(K + 2) u < 1, i.e. K < 4000) gamma_{K+1} <= (K + 2) u, hence
        |got - ref| <= (K + 2) u S.
  * GELU and RESID.  The epilogue f is applied to the rounded x: |f(got_x) - f(x)| <= Lip(f) |got_x - x| with Lip = 1.13 for gelu_tanh
    (its derivative peaks at 1.129 near x = 1.46) and |gamma[m / rows_per_group][n]| for resid + x * gamma (1 without gamma).  The epilogue's
    own operations (RESID: one multiply and one add; GELU: a few operations whose result is relatively accurate to about an ulp) add
    relative roundings of the result: 2^-23 |ref| (two units u).  So
        |got - ref| <= Lip (K + 2) u S + 2^-23 |ref|.
    (The rounding of the gamma product is relative to |x gamma| <= |gamma| S, not to |ref|; the unit that (K + 2) holds beyond the K + 1
    roundings of the chain pays for it.)
  * gemm_qkv.  v and, without l2norm, k are x itself: the first bound, E = (K + 2) u S.  q without l2norm is x * plain_scale:
    |plain_scale| E + 2^-23 |ref|.  With l2norm a head's 64 channels are normalised, r = x / max(||x||, 1e-12) (q: times exp(min(scale_mul,
    ln 100))).  For any two vectors ||x/||x|| - y/||y|| || <= 2 ||x - y|| / ||x|| (Dunkl and Williams 1964), so every channel of the head is
    within 2 ||E||_2 / ||x|| of the exact normalisation of the exact x.  The fp32 normalisation's own roundings, counted on the result: the sum
    of squares is a sum of non-negative terms, one rounding per square and one per level of the 6-level butterfly, relative error <= 7 u, which
    the square root halves and rounds once more (<= 4.5 u); the division 1 u; for q the exponential (about an ulp = 2 u, the clamp is exact)
    and the product 1 u.  That is <= 8.5 u to first order; 16 u |ref| is taken, a factor below 2 for the second-order terms and the exponential.  So
        |got - ref| <= s (2 ||E||_2 / ||x||) + 16 u |ref|,   s = exp(min(scale_mul, ln 100)) for q, 1 for k.

None of these numbers is measured: they follow from K, the operands and the formats alone.
"""
import numpy as np

from var_amd import abi

U = 2.0 ** -24
SENTINEL_BITS = np.uint32(0x7FC5A5A5)                # a quiet NaN with a payload; neither the canonical NaN (0x7FC00000) nor the guard byte pattern
TAIL = 5                                             # NaN / sentinel elements behind the last addressed element of every allocation
GELU_C0, GELU_C1 = float(np.float32(0.7978845608028654)), float(np.float32(0.044715))       # the constants of vm_gelu_tanh as fp32 holds them
GELU_LIP = 1.13
LN100 = float(np.float32(4.605170249938965))
PICK_OF_TILE = {0: 0, 1: 1, 2: 2, 3: 4}              # varhip_gemm_force_tile value -> varhip_gemm_last_pick value (3 is k_gemm_any)
PICK_ANY = 3
TILE_DIMS = {0: (128, 128), 1: (128, 64), 2: (64, 64), 3: (32, 32)}       # varhip_gemm_force_tile value -> (BM, BN) of k_dma_gemm

M_VALUES, N_VALUES, K_VALUES = (1, 31, 33, 65, 129, 130), (4, 36, 68, 132, 260), (32, 256, 288)


def sentinel(n):
    return np.full(n, SENTINEL_BITS, np.uint32).view(np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def gelu_tanh64(x):
    u = GELU_C0 * (x + GELU_C1 * (x * x) * x)
    return x / (1.0 + np.exp(-2.0 * u))


# ---------------------------------------------------------------------------------------------------------------------
# cases
def nt(name, M, N, K, epi=0, tile=-1, pick=None, evec=None, **kw):
    """one varhip_gemm_nt_f32 call.  Geometry keys (defaults dense): lda ldw ldo ldr ldg, offA offW offO offB offR offG (element offsets of
    the pointers), batch, sA sW sO (None: the dense stride; 0 shares the operand), bias / gamma (False: NULL), rpg, bpr (bias_per_row).
    tile: the forced tile (-1 automatic), pick: the varhip_gemm_last_pick value the call must report (None: not asserted), evec: the
    varhip_gemm_last_evec value it must report (None: 1 on a tile, -1 on the fallback; not asserted without pick)."""
    if evec is None and pick is not None:
        evec = -1 if pick == PICK_ANY else 1
    c = dict(kind='nt', name=name, M=M, N=N, K=K, epi=epi, tile=tile, pick=pick, evec=evec, lda=K, ldw=K, ldo=N, ldr=N, ldg=N, offA=0, offW=0, offO=0, offB=0,
             offR=0, offG=0, batch=1, sA=None, sW=None, sO=None, bias=True, gamma=True, rpg=1, bpr=0, einval=False)
    unknown = set(kw) - set(c)
    assert not unknown, unknown
    c.update(kw)
    for s, rows, ld in (('sA', M, 'lda'), ('sW', N, 'ldw'), ('sO', M, 'ldo')):
        if c[s] is None:
            c[s] = rows * c[ld] if c['batch'] > 1 else 0
    return c


def _triples(seed, n=12):
    """n (M, N, K) triples that cover every value of M_VALUES, N_VALUES and K_VALUES (n >= 6): each list is repeated up to n and shuffled"""
    rs = np.random.default_rng(seed)
    cols = []
    for vals in (M_VALUES, N_VALUES, K_VALUES):
        col = [vals[i % len(vals)] for i in range(n)]
        rs.shuffle(col)
        cols.append(col)
    out = list(zip(*cols))
    assert all(set(col) == set(vals) for col, vals in zip(cols, (M_VALUES, N_VALUES, K_VALUES)))
    return out


def ragged_cases():
    """every tile on 12 seeded ragged triples and all three epilogues; bias NULL on every fourth case, gamma NULL on every third RESID case,
    rows_per_group = 7 (divides none of the M values above 1); plus one forced call with K = 40 per tile, which must take the fallback"""
    out = []
    for tile in range(4):
        for i, (M, N, K) in enumerate(_triples(1000 + tile)):
            for epi in (0, 1, 2):
                out.append(nt(f'ragged t{tile} {M}x{N}x{K} e{epi}', M, N, K, epi, tile, PICK_OF_TILE[tile], bias=(i + epi) % 4 != 1,
                              gamma=(i % 3 != 0), rpg=7))
        out.append(nt(f'ragged t{tile} forced, K=40', 130, 68, 40, tile % 3, tile, PICK_ANY, rpg=7))
    return out


def vec_cases():
    """every condition of the fast path broken alone from a base that passes (130x68x64 on forced tile 2), and the controls that keep it"""
    M, N, K, t = 130, 68, 64, 2
    brk = [('lda=K+1', dict(lda=K + 1)), ('ldw=K+2', dict(ldw=K + 2)), ('A+1', dict(offA=1)), ('A+2', dict(offA=2)), ('A+3', dict(offA=3)),
           ('W+1', dict(offW=1)), ('sA=M*lda+1', dict(batch=2, sA=M * K + 1)), ('sW=N*ldw+2', dict(batch=2, sW=N * K + 2)), ('K=40', dict(K=40))]
    keep = [('base', {}), ('lda=K+4', dict(lda=K + 4)), ('ldw=K+8', dict(ldw=K + 8)), ('A+4', dict(offA=4)),
            ('sA+4', dict(batch=2, sA=M * K + 4)), ('sW+4', dict(batch=2, sW=N * K + 4))]
    out = []
    for lst, pick in ((brk, PICK_ANY), (keep, PICK_OF_TILE[t])):
        for i, (nm, kw) in enumerate(lst):
            kw = dict(kw)
            Kc = kw.pop('K', K)
            for key in ('lda', 'ldw'):                       # (the K = 40 case keeps dense rows)
                kw.setdefault(key, Kc)
            batched = kw.get('batch', 1) > 1
            for epi in ((0, 1) if batched else (0, 1, 2)):    # resid / gamma exist with batch == 1 only
                out.append(nt(f'vec {nm} e{epi}', M, N, Kc, epi, t, pick, rpg=7, **kw))
    return out


def evec_cases():
    """every condition of the vector epilogue broken alone (varhip_gemm_last_evec must report 0), on each tile, at 65x36 and 129x132 (partial
    tiles in both dimensions; K = 64), and the padded controls that keep it (1).  k_dma_gemm has three epilogues: the lean one of full tiles
    (evec, a column bias, the tile inside M x N), the general loop with 16-byte accesses (evec, every other tile) and the general loop element
    by element (not evec, and the ragged last columns).  129x132 holds a full tile of every size and 65x36 of the 32x32 one, and both have
    partial tiles, so the controls put padded ldo / ldr / ldg through the first two on every tile and the broken cases through the third."""
    out = []
    for tile in range(4):
        for M, N in ((65, 36), (129, 132)):
            K = 64
            brk = [('N=33', dict(N=33, ldo=36, ldr=36, ldg=36), None), ('ldo=N+1', dict(ldo=N + 1), None), ('out+1', dict(offO=1), None), ('bias+1', dict(offB=1), None),
                   ('ldr=N+2', dict(ldr=N + 2), 2), ('resid+3', dict(offR=3), 2), ('ldg=N+1', dict(ldg=N + 1), 2), ('gamma+1', dict(offG=1), 2),
                   ('sO=M*ldo+1', dict(batch=2, sO=M * N + 1), 0)]
            for i, (nm, kw, epi) in enumerate(brk):
                kw = dict(kw)
                Nc = kw.pop('N', N)
                for key in ('ldo', 'ldr', 'ldg'):
                    kw.setdefault(key, Nc)
                e = (i + tile) % 3 if epi is None else ((i + tile) % 2 if epi == 0 else epi)
                out.append(nt(f'evec t{tile} {M}x{Nc} {nm} e{e}', M, Nc, K, e, tile, PICK_OF_TILE[tile], 0, rpg=7, **kw))
            ctl = [('ctl ldo=N+4', dict(ldo=N + 4), (0, 1, 2)), ('ctl ldr=N+8', dict(ldr=N + 8), (2,)), ('ctl ldg=2N gamma+N', dict(ldg=2 * N, offG=N), (2,)),
                   ('ctl all padded', dict(ldo=N + 4, ldr=N + 8, ldg=2 * N, offG=N, offO=4, offB=4, offR=8), (2,)),
                   ('ctl sO=M*ldo+4', dict(batch=2, sO=M * N + 4), (0, 1))]
            for nm, kw, epis in ctl:
                for e in epis:
                    out.append(nt(f'evec t{tile} {M}x{N} {nm} e{e}', M, N, K, e, tile, PICK_OF_TILE[tile], 1, rpg=7, **kw))
    return out


def fallback_cases():
    """k_gemm_any has an epilogue of its own (ldo, ldr, ldg and the row group of gamma): K = 40 sends the evec geometries to it, with padded and
    odd leading dimensions of every operand, interior pointers and a padded batch stride"""
    out = []
    for M, N in ((65, 36), (129, 132)):
        K = 40
        geo = [('ldo=N+4', dict(ldo=N + 4), (0, 1, 2)), ('ldo=N+1', dict(ldo=N + 1), (0, 1, 2)), ('ldr=N+8', dict(ldr=N + 8), (2,)), ('ldr=N+2', dict(ldr=N + 2), (2,)),
               ('ldg=2N gamma+N', dict(ldg=2 * N, offG=N), (2,)), ('ldg=N+1', dict(ldg=N + 1), (2,)),
               ('all padded', dict(lda=K + 3, ldw=K + 5, ldo=N + 4, ldr=N + 8, ldg=2 * N, offA=1, offW=2, offO=1, offB=3, offR=2, offG=N), (2,)),
               ('lda=K+3 ldw=K+5', dict(lda=K + 3, ldw=K + 5), (0,)), ('sO=M*ldo+5 ldo=N+3', dict(batch=2, ldo=N + 3, sO=M * (N + 3) + 5), (0, 1))]
        for nm, kw, epis in geo:
            for e in epis:
                out.append(nt(f'fallback {M}x{N}x{K} {nm} e{e}', M, N, K, e, 2, PICK_ANY, rpg=7, **kw))
    return out


def batched_cases():
    """batch 2 and 3 on every tile and on the fallback (K = 40): shared / own A x shared / own W, sO padded beyond M * ldo, bias per row and
    per column, epi NONE and GELU, 33x68 and 130x36"""
    out = []
    i = 0
    for tile in (0, 1, 2, 3, None):
        K = 64 if tile is not None else 40
        for batch in (2, 3):
            for sa in (0, 1):
                for sw in (0, 1):
                    for bpr in (0, 1):
                        for epi in (0, 1):
                            M, N = ((33, 68), (130, 36))[(i + i // 2) & 1]
                            i += 1
                            out.append(nt(f'batched t{tile} b{batch} sA{sa} sW{sw} bpr{bpr} {M}x{N} e{epi}', M, N, K, epi,
                                          tile if tile is not None else 1, PICK_OF_TILE[tile] if tile is not None else PICK_ANY,
                                          batch=batch, sA=(M * K + 4) * sa, sW=(N * K + 8) * sw, sO=M * N + 4 * (1 + i % 2), bpr=bpr))
    return out


def einval_cases():
    """batch > 1 with resid or gamma: refused, `out` untouched"""
    return [nt('batch 2 with resid', 33, 68, 64, 2, batch=2, gamma=False, einval=True),
            nt('batch 2 with resid and gamma', 33, 68, 64, 2, batch=2, einval=True),
            nt('batch 3 with gamma only', 33, 68, 64, 0, batch=3, einval='gamma')]


QKV_SHAPES = [(4, 1, 2, 128, 0, 14, 1), (4, 9, 2, 128, 5, 14, 1), (2, 16, 16, 1024, 14, 55, 1), (4, 4, 3, 192, 1, 14, 0), (6, 100, 5, 320, 30, 130, 1),
              (128, 4, 16, 1024, 1, 5, 1), (3, 169, 1, 64, 0, 169, 1), (1, 1, 3, 192, 4, 5, 1), (2, 1, 1, 64, 0, 1, 0)]      # test_gemm_qkv_fused_epilogue_exact's list


def qkv(name, B2, l, H, K, pos0, Lmax, l2, tile=-1, **kw):
    c = dict(kind='qkv', name=name, B2=B2, l=l, H=H, K=K, pos0=pos0, Lmax=Lmax, l2=l2, tile=tile, pick=tile if tile >= 0 else None, lda=K, ldw=K)
    c.update(kw)
    return c


def qkv_cases():
    out = []
    for tile in (0, 1):
        for s in QKV_SHAPES:
            out.append(qkv(f'qkv t{tile} {s}', *s, tile=tile))
        out.append(qkv(f'qkv t{tile} lda=K+4', 4, 9, 2, 128, 5, 14, 1, tile=tile, lda=132))
        out.append(qkv(f'qkv t{tile} ldw=K+8', 3, 50, 3, 96, 7, 60, 0, tile=tile, ldw=104))
    return out


GROUPS = {'ragged': ragged_cases, 'vec': vec_cases, 'evec': evec_cases, 'fallback': fallback_cases, 'batched': batched_cases, 'qkv': qkv_cases}


# ---------------------------------------------------------------------------------------------------------------------
# operands
def _alloc(rng, off, batch, stride, rows, ld, cols, scale):
    """-> (flat fp32 allocation, all NaN but the real elements; view of the real elements [batch][rows][cols] as float64)"""
    nb = batch if stride else 1
    n = off + (nb - 1) * stride + (rows - 1) * ld + cols + TAIL
    flat = np.full(n, np.nan, np.float32)
    real = (rng.standard_normal((nb, rows, cols)) * scale).astype(np.float32)
    for b in range(nb):
        for r in range(rows):
            s = off + b * stride + r * ld
            flat[s:s + cols] = real[b, r]
    if nb < batch:
        real = np.broadcast_to(real, (batch, rows, cols))
    return flat, real.astype(np.float64)


class Built:
    pass


def build_nt(c, seed=0):
    rng = np.random.default_rng(seed)
    M, N, K, batch = c['M'], c['N'], c['K'], c['batch']
    b = Built()
    b.case = c
    b.A, b.A64 = _alloc(rng, c['offA'], batch, c['sA'], M, c['lda'], K, 1.0)
    b.W, b.W64 = _alloc(rng, c['offW'], batch, c['sW'], N, c['ldw'], K, 0.05)
    nbias = M if c['bpr'] else N
    b.bias, bias64 = _alloc(rng, c['offB'], 1, 0, 1, nbias, nbias, 0.1)
    b.bias64 = bias64[0, 0] if c['bias'] else None
    b.resid, resid64 = _alloc(rng, c['offR'], 1, 0, M, c['ldr'], N, 1.0)
    G = (M + c['rpg'] - 1) // c['rpg']
    b.gamma, gamma64 = _alloc(rng, c['offG'], 1, 0, G, c['ldg'], N, 1.0)
    use_resid = c['epi'] == abi.EPI_RESID or c['einval'] is True
    use_gamma = (c['epi'] == abi.EPI_RESID and c['gamma']) or (c['einval'] is True and c['gamma']) or c['einval'] == 'gamma'
    b.resid64 = resid64[0] if use_resid else None
    b.gamma64 = gamma64[0][np.arange(M) // c['rpg']] if use_gamma else None         # [M][N]: the row's group
    b.out = sentinel(c['offO'] + (batch - 1) * c['sO'] + (M - 1) * c['ldo'] + N + TAIL)
    b.inside = np.zeros(b.out.size, bool)
    for bb in range(batch):
        for r in range(M):
            s = c['offO'] + bb * c['sO'] + r * c['ldo']
            b.inside[s:s + N] = True
    def ptr(arr, off):
        return (arr, off) if off else arr
    b.args = [ptr(b.A, c['offA']), c['lda'], ptr(b.W, c['offW']), c['ldw'], ptr(b.bias, c['offB']) if c['bias'] else None,
              ptr(b.out, c['offO']), c['ldo'], M, N, K, c['epi'], ptr(b.resid, c['offR']) if use_resid else None, c['ldr'],
              ptr(b.gamma, c['offG']) if use_gamma else None, c['ldg'], c['rpg'], c['bpr'], batch, c['sA'], c['sW'], c['sO']]
    b.name, b.outs = 'gemm_nt_f32', [5]
    return b


def reference_nt(A64, W64, bias64, epi, resid64=None, gamma64=None, bias_per_row=0):
    """A64 [batch][M][K], W64 [batch][N][K] -> (ref, bound) [batch][M][N] float64 (module docstring)"""
    K = A64.shape[-1]
    x = A64 @ np.swapaxes(W64, -1, -2)
    S = np.abs(A64) @ np.swapaxes(np.abs(W64), -1, -2)
    if bias64 is not None:
        bb = bias64[:, None] if bias_per_row else bias64[None, :]
        x = x + bb
        S = S + np.abs(bb)
    E = (K + 2) * U * S
    if epi == abi.EPI_NONE:
        return x, E
    if epi == abi.EPI_GELU:
        ref = gelu_tanh64(x)
        return ref, GELU_LIP * E + 2.0 ** -23 * np.abs(ref)
    ref = resid64 + (x * gamma64 if gamma64 is not None else x)
    return ref, (np.abs(gamma64) if gamma64 is not None else 1.0) * E + 2.0 ** -23 * np.abs(ref)


def _within(name, got, ref, bound):
    err = np.abs(got.astype(np.float64) - ref)
    bad = ~(err <= bound)
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f'{name}: max err / bound = {ratio:.3f}')
    assert not bad.any(), (f'{name}: {int(bad.sum())}/{bad.size} outside the float64 bound, first at {tuple(np.argwhere(bad)[0])}: got '
                           f'{got[tuple(np.argwhere(bad)[0])]!r} ref {ref[tuple(np.argwhere(bad)[0])]!r} bound {bound[tuple(np.argwhere(bad)[0])]:.3e}')


def verify_nt(b, out):
    """the sentinel / padding conditions and the float64 bound on the `out` allocation a call on build_nt(c)'s operands left"""
    c = b.case
    out = np.asarray(out).reshape(-1)
    ob = bits(out)
    pad_changed = np.flatnonzero((ob != SENTINEL_BITS) & ~b.inside)
    assert pad_changed.size == 0, f"{c['name']}: {pad_changed.size} padding elements of out were written, first at element {int(pad_changed[0])}"
    if c['einval']:
        assert bool((ob == SENTINEL_BITS).all()), f"{c['name']}: a refused call wrote to out"
        return
    missed = np.flatnonzero((ob == SENTINEL_BITS) & b.inside)
    assert missed.size == 0, f"{c['name']}: {missed.size} elements inside [M][N] were not written, first at element {int(missed[0])}"
    M, N, batch = c['M'], c['N'], c['batch']
    got = np.empty((batch, M, N), np.float32)
    for bb in range(batch):
        for r in range(M):
            s = c['offO'] + bb * c['sO'] + r * c['ldo']
            got[bb, r] = out[s:s + N]
    nonfinite = np.argwhere(~np.isfinite(got))
    assert nonfinite.size == 0, f"{c['name']}: {len(nonfinite)} non-finite results (a padding element was read?), first at {tuple(nonfinite[0])}"
    ref, bound = reference_nt(b.A64, b.W64, b.bias64, c['epi'], b.resid64, b.gamma64, c['bpr'])
    _within(c['name'], got, ref, bound)


def build_qkv(c, seed=0):
    rng = np.random.default_rng(seed)
    B2, l, H, K, Lmax = c['B2'], c['l'], c['H'], c['K'], c['Lmax']
    C, M = 64 * H, B2 * l
    b = Built()
    b.case = c
    b.A, b.A64 = _alloc(rng, 0, 1, 0, M, c['lda'], K, 1.0)
    b.W, b.W64 = _alloc(rng, 0, 1, 0, 3 * C, c['ldw'], K, 0.05)
    b.bias = (rng.standard_normal(3 * C) * 0.1).astype(np.float32)
    b.sm = (np.log(4.0) + rng.standard_normal(H) * 0.5).astype(np.float32)
    b.sm[0] = 6.0                                            # exercises the clamp at ln 100
    b.plain = 0.03125
    b.q = sentinel(M * C).reshape(M, C)
    b.kc = sentinel(B2 * H * Lmax * 64).reshape(B2, H, Lmax, 64)
    b.vc = sentinel(B2 * H * Lmax * 64).reshape(B2, H, Lmax, 64)
    b.args = [b.A, c['lda'], b.W, c['ldw'], b.bias, M, C, K, b.sm if c['l2'] else None, b.plain, c['l2'], b.q, b.kc, b.vc, B2, l, H, c['pos0'], Lmax]
    b.name, b.outs = 'gemm_qkv_f32', [11, 12, 13]
    return b


def reference_qkv(b):
    """-> ((q, k, v) references, (q, k, v) bounds), q [M][C], k / v [B2][H][l][64] (the rows the call appends to the caches)"""
    c = b.case
    B2, l, H, K = c['B2'], c['l'], c['H'], c['K']
    C, M = 64 * H, B2 * l
    bias64 = b.bias.astype(np.float64)
    x = b.A64[0] @ b.W64[0].T + bias64
    E = (K + 2) * U * (np.abs(b.A64[0]) @ np.abs(b.W64[0]).T + np.abs(bias64))
    xs = [x[:, i * C:(i + 1) * C].reshape(M, H, 64) for i in range(3)]
    Es = [E[:, i * C:(i + 1) * C].reshape(M, H, 64) for i in range(3)]
    if c['l2']:
        s = np.exp(np.minimum(b.sm.astype(np.float64), LN100))[None, :, None]
        refs, bnds = [], []
        for i, scale in ((0, s), (1, 1.0)):
            nrm = np.maximum(np.sqrt((xs[i] ** 2).sum(-1, keepdims=True)), 1e-12)
            r = xs[i] / nrm * scale
            refs.append(r)
            bnds.append(scale * 2.0 * np.sqrt((Es[i] ** 2).sum(-1, keepdims=True)) / nrm + 16 * U * np.abs(r))
        qr, kr = refs
        qb, kb = bnds
    else:
        qr = xs[0] * b.plain
        qb = abs(b.plain) * Es[0] + 2.0 ** -23 * np.abs(qr)
        kr, kb = xs[1], Es[1]
    def cache(t):                                             # [M][H][64] -> [B2][H][l][64]
        return np.ascontiguousarray(np.broadcast_to(t, (M, H, 64)).reshape(B2, l, H, 64).transpose(0, 2, 1, 3))
    return (qr.reshape(M, C), cache(kr), cache(xs[2])), (np.broadcast_to(qb, (M, H, 64)).reshape(M, C), cache(kb), cache(Es[2]))


def verify_qkv(b, q, kc, vc):
    c = b.case
    l, pos0 = c['l'], c['pos0']
    refs, bnds = reference_qkv(b)
    q, kc, vc = np.asarray(q), np.asarray(kc), np.asarray(vc)
    assert not (bits(q) == SENTINEL_BITS).any(), f"{c['name']}: elements of q_out were not written"
    assert np.isfinite(q).all(), f"{c['name']}: non-finite q (a padding element was read?)"
    _within(c['name'] + ' q', q, refs[0], bnds[0])
    for nm, cache, ref, bnd in (('kcache', kc, refs[1], bnds[1]), ('vcache', vc, refs[2], bnds[2])):
        rows = np.zeros(c['Lmax'], bool)
        rows[pos0:pos0 + l] = True
        cb = bits(cache)
        assert bool((cb[:, :, ~rows] == SENTINEL_BITS).all()), f"{c['name']}: {nm} changed outside positions [{pos0}, {pos0 + l})"
        new = cache[:, :, rows]
        assert not (bits(new) == SENTINEL_BITS).any() and np.isfinite(new).all(), f"{c['name']}: {nm} rows not written or not finite"
        _within(f"{c['name']} {nm}", new, ref, bnd)


def build(c, seed=0):
    return build_nt(c, seed) if c['kind'] == 'nt' else build_qkv(c, seed)


def run_case(c, call, seed=0):
    """build the case's operands, call(case, name, args, outs) -> the output arrays after the call, verify them"""
    b = build(c, seed)
    res = call(c, b.name, b.args, b.outs)
    if c['kind'] == 'nt':
        verify_nt(b, res[0])
    else:
        verify_qkv(b, *res)
    return b, res


def host_call(L):
    """call(...) of run_case for the twins alone: varref_<name> of the bound oracle library L on guarded host arenas (the host half of
    tests/test_kernels_gpu.py::both)"""
    from tests import util

    def call(c, name, args, outs):
        copies, arrays, ptrs = {}, [], []
        for a in args:
            off = 0
            if isinstance(a, tuple):
                a, off = a
            if isinstance(a, np.ndarray):
                ra = copies.setdefault(id(a), np.ascontiguousarray(a).copy())
                arrays.append(ra); ptrs.append(ra.reshape(-1)[off:])
            else:
                arrays.append(None); ptrs.append(a)
        rc = util.guarded_invoke(f'varref_{name}', ptrs, L[name])
        assert rc == (abi.EINVAL if c.get('einval') else 0), f'oracle {name} rc={rc}'
        return [arrays[i] for i in outs]
    return call


# ---------------------------------------------------------------------------------------------------------------------
# the VAE AttnBlock's four products (var_amd/engine.py, attnblock) at a ragged size: interior pointers, lda = ldw = 2 Cc, batch strides
def attn_chain(call, Cc=32, HW=36, B=2, tile=-1, seed=0):
    """call(case, name, args, outs) as in run_case; the case dicts here carry name / tile / pick only.  Each product is checked against
    float64 on the operands it was given (the previous product's fp32 result), so the chain's steps are pinned one by one."""
    rng = np.random.default_rng(seed + HW)
    M = B * HW
    xn = rng.standard_normal((M, Cc)).astype(np.float32)
    wqkv = (rng.standard_normal((3 * Cc, Cc)) * 0.05).astype(np.float32)
    bqkv = (rng.standard_normal(3 * Cc) * 0.1).astype(np.float32)
    forced = PICK_OF_TILE[tile] if tile >= 0 else None
    def step(nm, args, shape, A64, W64, bias64, bpr, pick):
        out = sentinel(int(np.prod(shape))).reshape(shape)
        args[5] = out
        (res,) = call(dict(kind='nt', name=f'attn HW={HW} t{tile} {nm}', tile=tile, pick=pick, evec=None), 'gemm_nt_f32', args, [5])
        res = np.asarray(res).reshape(shape)
        assert not (bits(res) == SENTINEL_BITS).any() and np.isfinite(res).all(), f'attn {nm}: out not written or not finite'
        ref, bound = reference_nt(A64, W64, bias64, abi.EPI_NONE, bias_per_row=bpr)
        _within(f'attn HW={HW} t{tile} {nm}', res.reshape(ref.shape), ref, bound)
        return res
    x64, w64, b64 = xn.astype(np.float64), wqkv.astype(np.float64), bqkv.astype(np.float64)
    qk = step('qk', [xn, Cc, wqkv, Cc, bqkv, None, 2 * Cc, M, 2 * Cc, Cc, 0, None, 0, None, 0, 1, 0, 1, 0, 0, 0], (M, 2 * Cc),
              x64[None], w64[None, :2 * Cc], b64[:2 * Cc], 0, forced)
    vt = step('v^T', [(wqkv, 2 * Cc * Cc), Cc, xn, Cc, (bqkv, 2 * Cc), None, HW, Cc, HW, Cc, 0, None, 0, None, 0, 1, 1, B, 0, HW * Cc, Cc * HW],
              (B, Cc, HW), np.broadcast_to(w64[2 * Cc:], (B, Cc, Cc)), x64.reshape(B, HW, Cc), b64[2 * Cc:], 1, forced)
    qk64 = qk.astype(np.float64).reshape(B, HW, 2 * Cc)
    s = step('q.k^T', [qk, 2 * Cc, (qk, Cc), 2 * Cc, None, None, HW, HW, HW, Cc, 0, None, 0, None, 0, 1, 0, B, HW * 2 * Cc, HW * 2 * Cc, HW * HW],
             (B, HW, HW), qk64[:, :, :Cc], qk64[:, :, Cc:], None, 0, forced)
    z = s.astype(np.float64) * Cc ** -0.5
    p = np.exp(z - z.max(-1, keepdims=True))
    p = (p / p.sum(-1, keepdims=True)).astype(np.float32)
    step('p.v', [p, HW, vt, HW, None, None, Cc, HW, Cc, HW, 0, None, 0, None, 0, 1, 0, B, HW * HW, Cc * HW, HW * Cc], (B, HW, Cc),
         p.astype(np.float64), vt.astype(np.float64), None, 0, (forced if HW % 32 == 0 else PICK_ANY) if tile >= 0 else None)


def gemm16_tolerance(mag, ref, out16, gamma_abs=None, ulp16=2.0 ** -10):
    """the tolerance of tests/test_f16_gpu.py::test_gemm16_against_float64 (mag = |A| @ |W|^T on the 16-bit inputs): fp32 accumulation noise,
    one 16-bit rounding of a 16-bit result (ulp16: 2^-10 for fp16 there, 2^-7 for bfloat16 in tests/test_bf16_gpu.py), the gate's factor and
    the residual add for RESID with gamma"""
    tol = 2e-6 * mag + 1e-6 + (np.abs(ref) * ulp16 if out16 else 0)
    if gamma_abs is not None:
        tol = tol * np.maximum(gamma_abs, 1.0) + 1e-6 * np.abs(ref)
    return tol
