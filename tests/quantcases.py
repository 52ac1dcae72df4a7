"""One case table, one operand builder and the float64 references of the quantizer step (var_amd/csrc/quant.hip and the edit forms of
var_amd/csrc/edit.hip), shared by tests/test_quant_dispatch_cpu.py (the oracle's twins alone) and tests/test_quant_dispatch_gpu.py (every kernel
route of the HIP library).  Every case names the route it must reach (varhip_quant_last_route, include/var_hip.h); the predicates of the
dispatch are restated here (phi_route, we_route, nc_route) so that a changed condition fails a test instead of silently moving cases.

Two references.  The twin in oracle/ walks the kernel's own fma chains: bit for bit.  The float64 reference is the operation as the model's
quant.py writes it, in float64 torch on the same fp32 operands: F.interpolate(mode='bicubic') (identity for pn == P), F.conv2d(padding=1),
up (1 - ratio) + conv ratio added to f_hat and subtracted from f_rest, F.interpolate(mode='area'), F.linear plus the level/position row.
The elementwise bars follow from the rounding points, u = 2^-24 (fp32 unit roundoff), first order in u (the second-order term is below
n u / 2 = 2e-5 of a bar):

  * bicubic map `up`.  Along one axis output o takes 4 taps at floor(src) - 1 .. + 2 (index-clamped) with the Keys cubic (A = -0.75) at
    t = src - floor(src), src = (pn / P)(o + 1/2) - 1/2.  The fp32 table (oracle.var_oracle.bicubic_taps, ATen's fp32 arithmetic) has
    src = fl(fl(fl(pn / P)(o + 1/2)) - 1/2): the rounded scale is off by u pn / P and is multiplied by o + 1/2 <= P, the product and the
    difference are each rounded at magnitude <= pn, and t = src - floor(src) once more below 1: |d src| <= (3 pn + 1) u — the "few 2^-24 P" of
    the tap position.  The weight of source pixel j is W(src - j) with W the Keys kernel, continuous and piecewise C1 with |W'| <= 1.35
    (|x| <= 1: 3.75 x^2 - 4.5 x, extreme -1.35 at x = 0.6; 1 < |x| < 2: |0.75 (3 x^2 - 10 x + 8)| <= 0.75), so the tap position moves each
    weight by at most 1.35 |d src|, also where floor(src) differs between the two (the weight that leaves and the one that enters are both
    W near +-2, i.e. near 0).  Evaluating the cubics in fp32 (Horner, seven roundings of intermediates no larger than 6, errors carried through
    factors x <= 2, arguments t + 1, 1 - t, 2 - t rounded) adds below 40 u per weight; 48 u is taken.  So per tap
        dw = 1.35 (3 pn + 1) u + 48 u,
    and with the dense [P][pn] operators M32 (the fp32 table, taps that clamp onto one pixel summed), M64 (the same in float64) and
    D = dw max(count32, count64) (the number of taps either table puts on pixel j):
        up32 - up64 = (M32 - M64) H M32^T + M64 H (M32 - M64)^T  (exactly), so
        |up32 - up64| <= D |H| |M32|^T + |M64| |H| D^T + 8 u |M32| |H| |M32|^T,
    the last term for the kernel's 2 x 4 roundings (one product and three fmas per pass).  pn == P: the bar is 0, `up` is H exactly.
  * f_hat, f_rest.  acc is one chain of at most 9 Cv fmas from 0, conv = acc + phi_b one rounding, hmix = up keep + conv ratio one rounding
    (the table's ratios 0, 0.5, 1 and keep = 1 - ratio make both products exact), f_hat + hmix one rounding: a term of the chain passes through
    at most n = 9 Cv + 3 roundings, phi_b through 3, up keep through 2 and the old f_hat through 1.  The flat form n u sum |terms| weighs
    every term with n; the bar here weighs each term with its own count, so it is never wider than the flat form:
        |got - ref| <= u [ (9 Cv + 3) ratio (|up| * |w|) + 3 ratio |phi_b| + 2 keep |up| + |f_hat_0| ]
                       + keep bar_up + ratio (bar_up * |w|),
    (* the 3x3 convolution with zero padding, |up| = |up64| + bar_up) the second line carrying the bicubic bar forward through |w|.
  * area pool.  s is a sequential sum over the window (n_w = (y1 - y0)(x1 - x0) elements, n_w - 1 roundings: 0 + f is exact) and two
    divisions (exact where the window side is a power of two): bar = n_w u sum |f| / n_w.  (With two inexact divisions the first two elements
    of a window see n_w + 1 roundings and every later one fewer; the flat n_w is kept as the bar.)
  * word embed.  One chain of Cv fmas, + word_b, + lvl_pos: bar = (Cv + 2) u (sum |pooled w| + |word_b| + |lvl_pos|); behind the pool
    (next_map) the pool's bar is carried forward through |w|.
  * nearest code.  d32 = (zz + ee) + (-2 dot): three chains of Cv fmas and two sums, each term of which is bounded by |z|^2 + |e|^2
    (2 sum |z e| <= |z|^2 + |e|^2): |d32 - d64| <= (Cv + 2) 2^-23 (|z|^2 + |e|^2) = E.  The returned code's float64 distance must be within E of
    the float64 minimum, and the code must BE the float64 argmin on every row whose runner-up is farther than E (with the larger |e| of the
    two); rows nearer than that are excused, at most 2 % per case.  The cosine flavour: the same with the normalised vectors (|z|^2 + |e|^2
    = 2; the normalisation's own roundings, about Cv / 2 + 3 per factor, stay inside the (Cv + 2) 2^-23 2).

None of these numbers is measured.  Every check prints max err / bar; tests/test_quant_dispatch_cpu.py asserts that no quantity's bar is vacuous
(the twin's largest ratio over the table is at least 0.01).
"""
import numpy as np

U = 2.0 ** -24
SENTINEL_BITS = np.uint32(0x7FC5A5A5)                # a quiet NaN with a payload; not the guard byte pattern
V = 64
SLOPE, W_EVAL = 1.35, 48.0
LDS_LIMIT = 64 * 1024
WE_ROWS = 16
ROUTE_PHI_LDS, ROUTE_PHI_PLAIN, ROUTE_WE32, ROUTE_WE_ANY, ROUTE_NC_MFMA, ROUTE_NC_ANY = 1, 2, 4, 8, 16, 32
PHI_ENTRIES = ('quant_accum', 'quant_accum_h', 'quant_residual', 'quant_accum_edit', 'quant_accum_h_edit')


def sentinel(*shape):
    return np.full(shape, SENTINEL_BITS, np.uint32).view(np.float32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch, restated
def phi_lds_bytes(Cv, P):
    """dynamic LDS of k_phi_accum_lds: the padded weights [Cv][9 Cv + 1] and three input rows with a halo [3][P + 2][Cv], fp32"""
    return 4 * (Cv * (9 * Cv + 1) + 3 * (P + 2) * Cv)


def phi_route(Cv, P, B, limit=LDS_LIMIT):
    return ROUTE_PHI_LDS if phi_lds_bytes(Cv, P) <= limit and B <= 65535 else ROUTE_PHI_PLAIN


def we_route(Cv, w_off, rows):
    """w_off: element offset of word_w from a 16-byte aligned address"""
    return ROUTE_WE32 if Cv == 32 and (4 * w_off) % 16 == 0 and (rows + WE_ROWS - 1) // WE_ROWS <= 65535 else ROUTE_WE_ANY


def nc_route(Cv, z_off, cb_off):
    return ROUTE_NC_MFMA if Cv == 32 and (4 * z_off) % 16 == 0 and (4 * cb_off) % 16 == 0 else ROUTE_NC_ANY


# ---------------------------------------------------------------------------------------------------------------------
# cases
def phi_cases():
    def c(Cv, P, pn, route, B=2, ratio=0.5):
        return dict(kind='phi', name=f'phi Cv={Cv} P={P} pn={pn} B={B} ratio={ratio}', Cv=Cv, P=P, pn=pn, B=B, ratio=ratio, route=route)
    L, N = ROUTE_PHI_LDS, ROUTE_PHI_PLAIN
    return [c(32, 32, 1, L), c(32, 32, 24, L), c(32, 32, 32, L),           # the 512-pixel pyramid: 50,048 B
            c(40, 14, 3, L), c(40, 14, 14, L),                             # 65,440 B, 96 under the limit
            c(42, 1, 1, L),                                                # the widest Cv that still fits
            c(8, 5, 2, L), c(8, 5, 2, L, ratio=0.0), c(8, 5, 2, L, ratio=1.0),      # P Cv = 40 < 256: idle threads behind the barrier
            c(33, 7, 4, L), c(33, 7, 4, L, B=3),                           # odd Cv: the padded weight stride is even
            c(1, 1, 1, L),
            c(40, 15, 3, N),                                               # 65,920 B: the first shape past the limit
            c(43, 1, 1, N),
            c(64, 3, 2, N), c(64, 3, 2, N, B=3), c(64, 3, 2, N, ratio=0.0), c(64, 3, 2, N, ratio=1.0),
            c(64, 16, 13, N),
            c(48, 9, 9, N)]


NEXT_PQ = [(32, 1), (32, 9), (32, 24), (32, 32), (15, 4), (14, 14), (3, 2)]


def next_cases():
    """next_map_f32 on every (P, pq) x Cv x C; word_w one element into its array on one case per Cv"""
    out = []
    for P, pq in NEXT_PQ:
        for Cv in (32, 40, 8):
            for C in (128, 300, 64):
                w_off = 1 if (P, pq, C) == (15, 4, 300) else 0
                out.append(dict(kind='next', name=f'next_map P={P} pq={pq} Cv={Cv} C={C} w+{w_off}', B=2, P=P, pq=pq, Cv=Cv, C=C, w_off=w_off,
                                route=ROUTE_WE32 if Cv == 32 and not w_off else ROUTE_WE_ANY))
    return out


def pool_cases():
    return [dict(kind='pool', name=f'area_pool P={P} pq={pq} Cv={Cv}', B=2 + (i == 2), P=P, pq=pq, Cv=Cv)
            for i, ((P, pq), Cv) in enumerate(zip(NEXT_PQ, (32, 40, 8, 40, 32, 8, 40)))]


def embed_cases():
    """word_embed_f32 alone.  B lq = 18: one full block of 16 rows that spans both images and a 2-row tail; 8: the zero-filled tail only"""
    out = []
    for B, lq in ((2, 9), (2, 4)):
        for C in (128, 300, 64):
            for Cv, w_off in ((32, 0), (32, 1), (40, 0), (8, 0)):
                out.append(dict(kind='embed', name=f'word_embed B={B} lq={lq} Cv={Cv} C={C} w+{w_off}', B=B, lq=lq, Cv=Cv, C=C, w_off=w_off,
                                route=ROUTE_WE32 if Cv == 32 and not w_off else ROUTE_WE_ANY))
    return out


def nearest_cases():
    out = []
    for cos in (False, True):
        for N in (1, 130):
            for Vn in (300, 512):
                for z_off, cb_off in ((0, 0), (1, 0), (0, 1)):
                    out.append(dict(kind='nearest', name=f"nearest{'_cos' if cos else ''} N={N} V={Vn} z+{z_off} cb+{cb_off}", cos=cos, N=N, V=Vn, Cv=32,
                                    z_off=z_off, cb_off=cb_off, route=ROUTE_NC_MFMA if not (z_off or cb_off) else ROUTE_NC_ANY))
    return out


def all_cases():
    return phi_cases() + next_cases() + pool_cases() + embed_cases() + nearest_cases()


# ---------------------------------------------------------------------------------------------------------------------
# operands
class Built:
    pass


def _rnd(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def build_phi(c):
    from oracle.var_oracle import bicubic_taps
    Cv, P, pn, B = c['Cv'], c['P'], c['pn'], c['B']
    rng = np.random.default_rng(1000 * Cv + 40 * P + pn + 7 * B)
    l = pn * pn
    b = Built()
    b.case, b.l, b.ld = c, l, l + 3
    b.cb = _rnd(rng, V, Cv)
    b.idx = rng.integers(0, V, (B, l)).astype(np.int64)
    b.h = _rnd(rng, B, l, Cv)
    # keep / gt rows are ld > pn * pn long; their padding would select code -1 (the band in front of the codebook: NaN)
    b.keep = np.ones((B, b.ld), np.uint8)
    b.keep[:, :l] = rng.random((B, l)) < 0.5
    b.keep[0, 0], b.keep[B - 1, l - 1] = 1, 0                                  # neither all-zero nor all-one
    b.gt = np.full((B, b.ld), -1, np.int64)
    b.gt[:, :l] = rng.integers(0, V, (B, l))
    k = b.keep[:, :l].astype(bool)
    b.sel = np.where(k, b.gt[:, :l], b.idx)
    b.h_sub = np.where(k[..., None], b.cb[b.gt[:, :l].clip(0)], b.h)
    b.ti, b.tw = bicubic_taps(pn, P) if pn != P else (None, None)
    b.pw = _rnd(rng, Cv, 3, 3, Cv, scale=(1.0 / (9 * Cv)) ** 0.5)
    b.pb = _rnd(rng, Cv, scale=0.05)
    b.f_hat0, b.f_rest0 = _rnd(rng, B, P, P, Cv), _rnd(rng, B, P, P, Cv)
    b.refs = {}
    return b


def phi_call(b, entry, side, Cv=None, pn=None, ld=None, null=(), refused=False):
    """-> (name, args, outs, what) of one entry point on the case's operands; side 'twin': the varref_ call that restates it (the edit forms:
    the plain twin on the substituted rows), side 'hip': the varhip_ call itself.  outs: positions of up, f_hat (and f_rest).
    Cv / pn / ld / null (names among ti, tw, f_rest, keep passed as NULL): the changed arguments of a call that must be refused; with
    `refused` f_hat and f_rest are sentinel-filled too, so that any store shows."""
    c = b.case
    B, P, r = c['B'], c['P'], c['ratio']
    up, f, fr = sentinel(B, P, P, c['Cv']), b.f_hat0.copy(), b.f_rest0.copy()
    if refused:
        f, fr = sentinel(*f.shape), sentinel(*fr.shape)
    tail = [None if 'ti' in null else b.ti, None if 'tw' in null else b.tw, b.pw, b.pb, r, up, f]
    dims = [B, c['pn'] if pn is None else pn, P, c['Cv'] if Cv is None else Cv]
    edit = entry.endswith('_edit')
    if entry == 'quant_residual':
        return 'quant_residual_f32', [b.idx, b.cb] + tail + [None if 'f_rest' in null else fr] + dims, [7, 8, 9], ('up', 'f_hat', 'f_rest')
    if edit and side == 'hip':
        src = b.h if entry == 'quant_accum_h_edit' else b.idx
        return (entry + '_f32', [src, None if 'keep' in null else b.keep, b.gt, b.ld if ld is None else ld, b.cb] + tail + dims, [10, 11],
                ('up', 'f_hat'))
    if entry in ('quant_accum_h', 'quant_accum_h_edit'):
        return 'quant_accum_h_f32', [b.h_sub if edit else b.h] + tail + dims, [6, 7], ('up', 'f_hat')
    return 'quant_accum_f32', [b.sel if edit else b.idx, b.cb] + tail + dims, [7, 8], ('up', 'f_hat')


def phi_hmap(b, entry):
    """the [B][pn][pn][Cv] map the entry point upsamples"""
    c = b.case
    if entry == 'quant_accum_h':
        h = b.h
    elif entry == 'quant_accum_h_edit':
        h = b.h_sub
    else:
        h = b.cb[b.sel if entry == 'quant_accum_edit' else b.idx]
    return h.reshape(c['B'], c['pn'], c['pn'], c['Cv'])


# ---------------------------------------------------------------------------------------------------------------------
# float64 references and bars (module docstring)
def keys_taps64(pn, P):
    A = -0.75
    idx, w = np.zeros((P, 4), np.int64), np.zeros((P, 4))
    for o in range(P):
        src = (pn / P) * (o + 0.5) - 0.5
        i0 = np.floor(src)
        t = src - i0
        c1 = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1
        c2 = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
        w[o] = [c2(t + 1), c1(t), c1(1 - t), c2(2 - t)]
        idx[o] = np.clip(int(i0) - 1 + np.arange(4), 0, pn - 1)
    return idx, w


def _dense(idx, w, pn):
    P = idx.shape[0]
    M, cnt = np.zeros((P, pn)), np.zeros((P, pn))
    rows = np.repeat(np.arange(P), 4)
    np.add.at(M, (rows, idx.reshape(-1)), np.asarray(w, np.float64).reshape(-1))
    np.add.at(cnt, (rows, idx.reshape(-1)), 1.0)
    return M, cnt


def _sep(My, H, Mx):
    return np.einsum('yi,bijc,xj->byxc', My, H, Mx)


def up_reference(hmap, pn, P, ti, tw):
    """-> (up64, bar) [B][P][P][Cv]"""
    import torch
    import torch.nn.functional as F
    h64 = hmap.astype(np.float64)
    if pn == P:
        return h64, np.zeros_like(h64)
    up = F.interpolate(torch.from_numpy(h64).permute(0, 3, 1, 2), size=(P, P), mode='bicubic', align_corners=False).permute(0, 2, 3, 1).numpy()
    M32, c32 = _dense(ti, tw, pn)
    M64, c64 = _dense(*keys_taps64(pn, P), pn)
    mine = _sep(M64, h64, M64)
    assert np.abs(mine - up).max() <= 1e-12 * (1 + np.abs(h64).max()), 'keys_taps64 is not the operator F.interpolate applies'
    dw = (SLOPE * (3 * pn + 1) + W_EVAL) * U
    D = dw * np.maximum(c32, c64)
    H = np.abs(h64)
    bar = _sep(D, H, np.abs(M32)) + _sep(np.abs(M64), H, D) + 8 * U * _sep(np.abs(M32), H, np.abs(M32))
    return up, bar


def _conv(x, w):
    """x [B][P][P][Cv], w [co][ky][kx][ci] float64 -> the 3x3 convolution with zero padding, [B][P][P][co]"""
    import torch
    import torch.nn.functional as F
    return F.conv2d(torch.from_numpy(np.ascontiguousarray(x)).permute(0, 3, 1, 2), torch.from_numpy(np.ascontiguousarray(w)).permute(0, 3, 1, 2),
                    padding=1).permute(0, 2, 3, 1).numpy()


def phi_reference(b, entry):
    """-> {'up': (ref, bar), 'f_hat': (ref, bar), 'f_rest': (ref, bar)}; cached per upsampled map"""
    key = {'quant_residual': 'quant_accum'}.get(entry, entry)
    if key in b.refs:
        return b.refs[key]
    c = b.case
    Cv, r = c['Cv'], float(np.float32(c['ratio']))
    keep = float(np.float32(1.0) - np.float32(c['ratio']))
    assert r in (0.0, 0.5, 1.0), 'the f_hat bar counts the two products of the mix as exact'
    up, bar_up = up_reference(phi_hmap(b, entry), c['pn'], c['P'], b.ti, b.tw)
    w64, b64 = b.pw.astype(np.float64), b.pb.astype(np.float64)
    conv = _conv(up, w64) + b64
    hmix = up * keep + conv * r
    aup = np.abs(up) + bar_up
    carried = keep * bar_up + r * _conv(bar_up, np.abs(w64))
    common = U * ((9 * Cv + 3) * r * _conv(aup, np.abs(w64)) + 3 * r * np.abs(b64) + 2 * keep * aup) + carried
    f0, fr0 = b.f_hat0.astype(np.float64), b.f_rest0.astype(np.float64)
    b.refs[key] = {'up': (up, bar_up), 'f_hat': (f0 + hmix, common + U * np.abs(f0)), 'f_rest': (fr0 - hmix, common + U * np.abs(fr0))}
    return b.refs[key]


def pool_reference(f, P, pq):
    """f [B][P][P][Cv] fp32 -> (pooled64, bar) [B][pq * pq][Cv]"""
    import torch
    import torch.nn.functional as F
    B, Cv = f.shape[0], f.shape[-1]
    f64 = torch.from_numpy(f.astype(np.float64)).permute(0, 3, 1, 2)
    area = lambda t: F.interpolate(t, size=(pq, pq), mode='area').permute(0, 2, 3, 1).reshape(B, pq * pq, Cv).numpy()
    side = np.array([((o + 1) * P + pq - 1) // pq - (o * P) // pq for o in range(pq)], np.float64)
    n_w = np.outer(side, side).reshape(1, pq * pq, 1)
    return area(f64), n_w * U * area(f64.abs())


def embed_reference(pooled64, bar_pool, ww, wb, lp, Cv):
    """-> (x64, bar) [B][lq][C] (both CFG halves hold it)"""
    import torch
    import torch.nn.functional as F
    w64, b64, lp64 = ww.astype(np.float64), wb.astype(np.float64), lp.astype(np.float64)
    x = F.linear(torch.from_numpy(pooled64), torch.from_numpy(w64), torch.from_numpy(b64)).numpy() + lp64[None]
    bar = (Cv + 2) * U * (np.abs(pooled64) @ np.abs(w64).T + np.abs(b64) + np.abs(lp64)[None]) + bar_pool @ np.abs(w64).T
    return x, bar


def within(name, got, ref, bar):
    """assert |got - ref| <= bar elementwise; prints and returns max err / bar"""
    got = np.asarray(got)
    assert got.shape == ref.shape, f'{name}: shape {got.shape} != {ref.shape}'
    assert not (bits(got) == SENTINEL_BITS).any(), f'{name}: elements were not written'
    assert np.isfinite(got).all(), f'{name}: non-finite results (a band or a padding element was read?)'
    err = np.abs(got.astype(np.float64) - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(err > 0, err / bar, 0.0)
    ratio = float(q.max()) if q.size else 0.0
    print(f'{name}: max err / bar = {ratio:.4f}')
    bad = ~(err <= bar)
    assert not bad.any(), (f'{name}: {int(bad.sum())}/{bad.size} outside the float64 bar (max err / bar = {ratio:.3f}), first at '
                           f'{tuple(np.argwhere(bad)[0])}: got {got[tuple(np.argwhere(bad)[0])]!r} ref {ref[tuple(np.argwhere(bad)[0])]!r}')
    return ratio


def build_next(c):
    rng = np.random.default_rng(100 * c['P'] + c['pq'] + 3 * c['Cv'] + c['C'])
    B, P, pq, Cv, C = c['B'], c['P'], c['pq'], c['Cv'], c['C']
    b = Built()
    b.case = c
    b.f = _rnd(rng, B, P, P, Cv)
    b.ww_flat = np.concatenate([np.full(c['w_off'], np.nan, np.float32), _rnd(rng, C * Cv, scale=0.2)])
    b.ww = b.ww_flat[c['w_off']:].reshape(C, Cv)
    b.wb, b.lp = _rnd(rng, C, scale=0.1), _rnd(rng, pq * pq, C)
    ww = (b.ww_flat, c['w_off']) if c['w_off'] else b.ww_flat
    b.args = [b.f, ww, b.wb, b.lp, sentinel(2 * B * pq * pq, C), sentinel(B, pq * pq, Cv), B, P, pq, C, Cv]
    b.name, b.outs = 'next_map_f32', [4, 5]
    return b


def verify_next(b, x, pooled):
    c = b.case
    B, lq, Cv = c['B'], c['pq'] ** 2, c['Cv']
    p64, pbar = pool_reference(b.f, c['P'], c['pq'])
    x64, xbar = embed_reference(p64, pbar, b.ww, b.wb, b.lp, Cv)
    x = np.asarray(x).reshape(2, B, lq, c['C'])
    assert np.array_equal(bits(x[0]), bits(x[1])), f"{c['name']}: the two CFG halves differ"
    return {'pooled': within(c['name'] + ' pooled', np.asarray(pooled).reshape(B, lq, Cv), p64, pbar),
            'x_out': max(within(c['name'] + f' x_out half {i}', x[i], x64, xbar) for i in (0, 1))}


def build_pool(c):
    rng = np.random.default_rng(100 * c['P'] + c['pq'] + c['Cv'])
    b = Built()
    b.case = c
    b.f = _rnd(rng, c['B'], c['P'], c['P'], c['Cv'])
    b.args = [b.f, sentinel(c['B'], c['pq'] ** 2, c['Cv']), c['B'], c['P'], c['pq'], c['Cv']]
    b.name, b.outs = 'area_pool_f32', [1]
    return b


def verify_pool(b, pooled):
    c = b.case
    p64, pbar = pool_reference(b.f, c['P'], c['pq'])
    return {'pooled': within(c['name'], np.asarray(pooled).reshape(p64.shape), p64, pbar)}


def build_embed(c):
    rng = np.random.default_rng(100 * c['lq'] + 3 * c['Cv'] + c['C'])           # (no w_off: the misaligned case holds the aligned one's values)
    B, lq, Cv, C = c['B'], c['lq'], c['Cv'], c['C']
    b = Built()
    b.case = c
    b.pooled = _rnd(rng, B, lq, Cv)
    b.ww_flat = np.concatenate([np.full(c['w_off'], np.nan, np.float32), _rnd(rng, C * Cv, scale=0.2)])
    b.ww = b.ww_flat[c['w_off']:].reshape(C, Cv)
    b.wb, b.lp = _rnd(rng, C, scale=0.1), _rnd(rng, lq, C)
    ww = (b.ww_flat, c['w_off']) if c['w_off'] else b.ww_flat
    b.args = [b.pooled, ww, b.wb, b.lp, sentinel(2 * B * lq, C), B, lq, C, Cv]
    b.name, b.outs = 'word_embed_f32', [4]
    return b


def verify_embed(b, x):
    c = b.case
    B, lq = c['B'], c['lq']
    p64 = b.pooled.astype(np.float64)
    x64, xbar = embed_reference(p64, np.zeros_like(p64), b.ww, b.wb, b.lp, c['Cv'])
    x = np.asarray(x).reshape(2, B, lq, c['C'])
    assert np.array_equal(bits(x[0]), bits(x[1])), f"{c['name']}: the two CFG halves differ"
    return {'x_out': max(within(c['name'] + f' half {i}', x[i], x64, xbar) for i in (0, 1))}


def build_nearest(c):
    rng = np.random.default_rng(17 * c['N'] + c['V'] + (5 if c['cos'] else 0))  # (no offsets: the misaligned cases hold the aligned one's values)
    N, Vn, Cv = c['N'], c['V'], c['Cv']
    b = Built()
    b.case = c
    z, cb = _rnd(rng, N, Cv, scale=1.5), _rnd(rng, Vn, Cv)
    if N > 3:
        cb[77] = cb[5]; z[3] = cb[5]                                           # an exact tie: the first index wins, the row is excused
    b.z_flat = np.concatenate([np.full(c['z_off'], np.nan, np.float32), z.reshape(-1)])
    b.cb_flat = np.concatenate([np.full(c['cb_off'], np.nan, np.float32), cb.reshape(-1)])
    b.z, b.cb = z, cb
    ptr = lambda a, off: (a, off) if off else a
    b.args = [ptr(b.z_flat, c['z_off']), ptr(b.cb_flat, c['cb_off']), np.full(N, -7, np.int64), N, Vn, Cv]
    b.name, b.outs = 'nearest_code_cos_f32' if c['cos'] else 'nearest_code_f32', [2]
    return b


def verify_nearest(b, idx):
    """-> the share of rows excused by the runner-up rule (module docstring)"""
    c = b.case
    N, Vn, Cv = c['N'], c['V'], c['Cv']
    idx = np.asarray(idx).reshape(-1)
    assert idx.shape == (N,) and ((idx >= 0) & (idx < Vn)).all(), f"{c['name']}: indices outside [0, V) or not written: {idx[:8]}"
    z, e = b.z.astype(np.float64), b.cb.astype(np.float64)
    if c['cos']:
        z = z / np.maximum(np.linalg.norm(z, axis=1, keepdims=True), 1e-12)
        e = e / np.maximum(np.linalg.norm(e, axis=1, keepdims=True), 1e-12)
        d = -(z @ e.T)
    else:
        d = ((z[:, None, :] - e[None, :, :]) ** 2).sum(-1)
    zz, ee = (z * z).sum(1), (e * e).sum(1)
    E = (Cv + 2) * 2.0 ** -23 * (zz[:, None] + ee[None, :])                    # [N][V]
    rows = np.arange(N)
    order = np.argsort(d, axis=1, kind='stable')
    best, second = order[:, 0], order[:, 1]
    over = d[rows, idx] - d[rows, best]
    ratio = float((over / E[rows, idx]).max())
    print(f"{c['name']}: max (d64[returned] - d64[min]) / E = {ratio:.4f}")
    assert (over <= E[rows, idx]).all(), f"{c['name']}: a returned code is farther than the fp32 bound from the float64 minimum (ratio {ratio:.3f})"
    decided = (d[rows, second] - d[rows, best]) > np.maximum(E[rows, best], E[rows, second])
    wrong = decided & (idx != best)
    assert not wrong.any(), f"{c['name']}: {int(wrong.sum())} rows with a clear float64 argmin returned another code, first row {int(np.flatnonzero(wrong)[0])}"
    excused = float((~decided).mean())
    print(f"{c['name']}: {int((~decided).sum())}/{N} rows excused by the runner-up rule")
    return excused


BUILD = {'next': build_next, 'pool': build_pool, 'embed': build_embed, 'nearest': build_nearest}
VERIFY = {'next': verify_next, 'pool': verify_pool, 'embed': verify_embed, 'nearest': verify_nearest}


# ---------------------------------------------------------------------------------------------------------------------
def host_call(L):
    """call(name, args, outs) -> the output arrays after varref_<name> ran on guarded host arenas (an arg may be (array, element_offset))"""
    from tests import util

    def call(name, args, outs, expect=0):
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
        assert rc == expect, f'oracle {name} rc={rc}'
        return [arrays[i] for i in outs]
    return call


def einval_phi_cases():
    """(name, entry, changes) on the base shape Cv = 8, P = 5, pn = 2, B = 2: every one must return VARHIP_EINVAL and write nothing.
    changes: {'Cv' / 'pn': value, 'null': names of the pointers passed as NULL, 'ld': value}"""
    out = []
    for entry in PHI_ENTRIES:
        out += [(f'{entry} Cv=65', entry, dict(Cv=65)), (f'{entry} Cv=0', entry, dict(Cv=0)), (f'{entry} pn>P', entry, dict(pn=6)),
                (f'{entry} null tap_idx', entry, dict(null=('ti',))), (f'{entry} null tap_w', entry, dict(null=('tw',)))]
        if entry == 'quant_residual':
            out.append((f'{entry} null f_rest', entry, dict(null=('f_rest',))))
        if entry.endswith('_edit'):
            out += [(f'{entry} ld_gt<pn*pn', entry, dict(ld=3)), (f'{entry} null keep', entry, dict(null=('keep',)))]
    return out

