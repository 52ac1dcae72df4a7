"""VAR.token_scores on the MI355X: varhip_code_dist_f32 against the neighbour table, varhip_token_score_f32 against float64 for every mode
(ties across group boundaries, underflowing tails, peaked rows), the end-to-end API against the engine's own d16 logits in every precision,
bitwise packing invariance, and no full logits tensor in memory.

Bars, from the kernel's rounding points (u = 2^-24):
  group_smoothed   exponentials (vm_exp, <= 2u each, plus u |z - m| <= 2u max|z| from the subtraction), the band sum (< G terms) and the row
                   sum s, two divisions, + 1e-10, then vm_log (about one ulp of a result of magnitude <= 23.1): to first order
                   u (G + n_s + 8) + 4u max|z| + 2u |result|, with n_s the additions one lane's part of s passes through (<= 85 at V = 5000).
                   Rounding errors of sums of positive terms add up far below their worst case; the tests assert the bar
                   1e-5 + 1e-6 max|z| at G <= 64.
  neighbor_max     (z_best - m) - log s: u |z_best - m| + (u n_s + one ulp of log s) + one ulp of the result <= 4u max|z| + u (n_s + 20), under
                   the same bar 1e-5 + 1e-6 max|z|.
  expected_distance  every term p_v d_v >= 0 carries a relative error of a few u (exponential, subtraction weighted by p, product) and the sums
                   of the numerator and denominator one of u n each: the result is within 1e-5 relative."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import util
from var_amd import abi, hip

pytestmark = pytest.mark.gpu

PNS16 = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
_M = {}
MODES = {'group_smoothed': 1, 'neighbor_max': 2, 'expected_distance': 3}


def d16():
    if 'd16' not in _M:
        from models import build_vae_var
        from var_amd.detinit import fill_module_device_
        with contextlib.redirect_stdout(io.StringIO()):
            vae, var = build_vae_var(device='cuda', patch_nums=PNS16, depth=16, ch=160)
        fill_module_device_(var, 16, 0, 'var.'); fill_module_device_(vae, 16, 0, 'vae.')
        var.eval(); vae.eval(); var.cond_drop_rate = 0.0
        _M['d16'] = (vae, var)
    return _M['d16']


def tokens(var, n, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    return torch.randint(0, var.V, (n, var.L), device='cuda', generator=g)


def restate64(z, g, score, par, dist):
    """float64 statement of the scores: z (R, V) fp32 rows, g (R,) tokens, dist (V, V) -> (R,) float64; order z descending, ties by index"""
    z64 = z.double()
    V = z.shape[-1]
    lp = z64.log_softmax(-1)
    p = lp.exp()
    if score == 'neighbor_max':
        return lp.masked_fill(dist[g].double() > par, -float('inf')).amax(-1)
    if score == 'expected_distance' and not par:
        return -(p * dist[g].double()).sum(-1)
    order = torch.sort(z64, dim=-1, descending=True, stable=True).indices
    if score == 'expected_distance':
        top = order[:, :par]
        pk = p.gather(1, top)
        return -(pk * dist[g].double().gather(1, top)).sum(-1) / pk.sum(-1)
    rank = (order == g.view(-1, 1)).int().argmax(-1)
    lo = rank - rank % par
    hi = torch.clamp(lo + par, max=V)
    ar = torch.arange(V, device=z.device).view(1, -1)
    band = (p.gather(1, order) * ((ar >= lo.view(-1, 1)) & (ar < hi.view(-1, 1)))).sum(-1)     # summed directly, in float64
    return torch.log(band / (hi - lo) + 1e-10)


def check(got, want, z, score):
    """the bars of the module docstring; z (R, V) -> (ok, max |diff|)"""
    diff = (got.double() - want).abs()
    if score == 'expected_distance':
        bar = 1e-5 * want.abs()
    else:
        bar = 1e-5 + 1e-6 * z.abs().amax(-1).double()
    return bool((diff <= bar).all()), float(diff.max())


def table(V, D=8, seed=0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    cb = torch.randn(V, D, device='cuda', generator=g)
    dist = torch.empty(V, V, device='cuda')
    util.guarded_call('code_dist_f32', cb, V, D, dist)
    return dist


def test_code_distance_table_matches_the_neighbour_table():
    vae, var = d16()
    eng = var.engine()
    dist = eng.code_distance_table()
    idx, nd = eng.neighbor_table(64)
    torch.cuda.synchronize()
    V = var.V
    assert dist.shape == (V, V) and dist.dtype == torch.float32
    assert torch.equal(dist.gather(1, idx.long()), nd), 'distance table differs from the neighbour table'
    assert bool((dist.diagonal() == 0).all())
    assert torch.equal(dist, dist.t()), 'distance table is not exactly symmetric'
    assert eng.code_distance_table() is dist                                 # cached


def make_rows(rows, V, g):
    """random logits with exact ties (values on a grid of 1/4), tails that underflow to p = 0 in fp32, and a few peaked rows"""
    z = torch.round(torch.randn(rows, V, device='cuda', generator=g) * 12) / 4
    z[1::4, : V // 3] -= 120                                                # tails with p = 0
    z[::5, :7] += 40                                                        # peaked rows
    z[2::6] = torch.round(z[2::6])                                          # coarse grid: long runs of ties across group boundaries
    return z


@pytest.mark.parametrize('V', [4096, 1000, 4099, 5000])
@pytest.mark.parametrize('cfg', [0.0, 1.5])
def test_kernel_vs_float64(V, cfg):
    """the pass layout of test_likelihood_gpu.py::test_kernel_vs_float64, every mode, written into a slice of a larger output"""
    _kernel_vs_float64(V, cfg, (3, 4, 7, 6, 20, 1, 9))


@pytest.mark.parametrize('V', [4096, 4099])
@pytest.mark.parametrize('cfg', [0.0, 1.5])
def test_kernel_vs_float64_slices_end_their_allocations(V, cfg):
    """the same with tok0 + l == L and k0 + classes == K: the last image's tokens are the last elements of gt, its last class row ends the output"""
    _kernel_vs_float64(V, cfg, (3, 4, 7, 6, 16, 2, 9))


def _kernel_vs_float64(V, cfg, layout):
    images, classes, l, K, L, k0, tok0 = layout
    u = 1 if cfg > 0 else 0
    g = torch.Generator(device='cuda').manual_seed(V + 7)
    rows = images * (classes + u) * l
    logits = make_rows(rows, V, g)
    if u:
        logits[images * classes * l:] = torch.round(logits[images * classes * l:])
    gt = torch.randint(0, V, (images, L), device='cuda', generator=g)
    t = np.float32(np.float32(cfg) * np.float32(0.5))
    ca, cb = np.float32(1) + t, t
    cond = logits[:images * classes * l].view(images, classes, l, V)
    if u:
        unc = logits[images * classes * l:].view(images, 1, l, V)
        z = torch.tensor(ca, device='cuda') * cond - torch.tensor(cb, device='cuda') * unc
    else:
        z = cond
    gsl = gt[:, tok0:tok0 + l]
    # ties with gt itself: some rows put gt's value on several other codes
    zrow = z.reshape(-1, V)
    gr = gsl.view(images, 1, l).expand(images, classes, l).reshape(-1)
    assert bool((zrow.gather(1, gr.view(-1, 1)) == zrow).sum(-1).gt(1).any())
    dist = table(V)
    thr = float(dist.median())
    cases = [('group_smoothed', 1), ('group_smoothed', 3), ('group_smoothed', 50), ('group_smoothed', 64), ('neighbor_max', 0.0),
             ('neighbor_max', thr), ('expected_distance', 0), ('expected_distance', 1), ('expected_distance', 37), ('expected_distance', V)]
    for score, par in cases:
        out = torch.full((images, K, L), 12345.0, device='cuda')
        ip = 0 if score == 'neighbor_max' else par
        util.guarded_call('token_score_f32', logits, gt[:, tok0:], L, images, classes, l, V, u, float(ca), float(cb), MODES[score], ip,
                 float(par) if score == 'neighbor_max' else 0.0, dist, V, out[:, k0:, tok0:], K * L, L)
        torch.cuda.synchronize()
        got = out[:, k0:k0 + classes, tok0:tok0 + l].reshape(-1)
        want = restate64(zrow, gr, score, par, dist)
        ok, err = check(got, want, zrow, score)
        assert ok, f'V={V} cfg={cfg} {score}({par}): max |diff| {err:.3e} beyond the bar'
        untouched = torch.ones_like(out, dtype=torch.bool)
        untouched[:, k0:k0 + classes, tok0:tok0 + l] = False
        assert bool((out[untouched] == 12345.0).all()), f'{score}: the kernel wrote outside its slice'


def test_kernel_rejects_bad_sizes():
    lg = torch.zeros(64, 256, device='cuda'); gt = torch.zeros(2, 8, dtype=torch.int64, device='cuda'); out = torch.zeros(2, 2, 8, device='cuda')
    dist = torch.zeros(256, 256, device='cuda')
    f = hip.lib().fn['token_score_f32']
    st = hip.current_stream()
    for mode, par, thr in ((1, 5, 0.0), (2, 0, 1.0), (3, 0, 0.0), (3, 256, 0.0)):
        good = [lg.data_ptr(), gt.data_ptr(), 8, 2, 2, 4, 256, 0, 1.0, 0.0, mode, par, thr, dist.data_ptr(), 256, out.data_ptr(), 16, 8]
        assert f(*good, st) == 0, mode
        torch.cuda.synchronize()
    good = [lg.data_ptr(), gt.data_ptr(), 8, 2, 2, 4, 256, 0, 1.0, 0.0, 3, 4, 0.0, dist.data_ptr(), 256, out.data_ptr(), 16, 8]
    for pos, val in [(3, 0), (4, 0), (5, 0), (6, 0), (2, 3), (17, 3), (16, 8), (0, None), (10, 0), (10, 4), (11, -1), (11, 257), (13, None),
                     (14, 255)]:
        a = list(good); a[pos] = val
        assert f(*a, st) == abi.EINVAL, (pos, val)
    for mode, par, thr in ((1, 0, 0.0), (2, 0, -1.0), (2, 0, float('inf')), (2, 0, float('nan'))):
        a = list(good); a[10], a[11], a[12] = mode, par, thr
        assert f(*a, st) == abi.EINVAL, (mode, par, thr)
    cd = hip.lib().fn['code_dist_f32']
    cbk = torch.zeros(16, 4, device='cuda')
    for args in ((None, 16, 4, dist.data_ptr()), (cbk.data_ptr(), 0, 4, dist.data_ptr()), (cbk.data_ptr(), 16, 0, dist.data_ptr()),
                 (cbk.data_ptr(), 16, 4, None)):
        assert cd(*args, st) == abi.EINVAL, args


def ref_rows(var, vae, gt, classes, cfg):
    """per image: the engine's own teacher-forced logits var(label, x), with guidance combined in fp32 -> (N, K, L, V) z"""
    x = vae.quantize.idxBl_to_var_input([gt[:, b:e] for b, e in var.begin_ends])
    S = len(var.patch_nums)
    ratio = torch.tensor([si / (S - 1) for si, pn in enumerate(var.patch_nums) for _ in range(pn * pn)], device='cuda')
    t = cfg * ratio.unsqueeze(0).unsqueeze(-1)
    zs = []
    for i in range(gt.shape[0]):
        z = var(torch.tensor(classes, device='cuda'), x[i:i + 1].expand(len(classes), -1, -1).contiguous())
        if cfg > 0:
            u = var(torch.tensor([var.num_classes], device='cuda'), x[i:i + 1].contiguous())
            z = (1 + t) * z - t * u
        zs.append(z)
    return torch.stack(zs)


D16_CASES = [('group_smoothed', dict(group=50), 50), ('neighbor_max', dict(threshold=None), None), ('expected_distance', dict(), 0),
             ('expected_distance', dict(top_k=100), 100)]


def d16_kw(var, kw):
    if 'threshold' in kw:
        d = var.engine().code_distance_table()
        return dict(threshold=float(d[:64].median()))
    return kw


@pytest.mark.parametrize('prec', ['f32', 'f16', 'bf16', 'auto'])
def test_d16_vs_engine_logits(prec):
    """L = 680, every mode, against the float64 statement on the engine's own teacher-forced logits of the same precision (cfg 0 and 1.5)"""
    vae, var = d16()
    gt = tokens(var, 2, 11)
    classes = [1, 207, 999]
    ctx = torch.autocast('cuda', dtype=torch.bfloat16) if prec == 'auto' else contextlib.nullcontext()
    var.set_hip_precision(prec)
    try:
        for cfg in (0.0, 1.5):
            with torch.no_grad(), ctx:
                z = ref_rows(var, vae, gt, classes, cfg).reshape(-1, var.V)
                res = {s: var.token_scores(gt, classes, s, cfg=cfg, **d16_kw(var, kw)) for s, kw, _ in D16_CASES[:3]}
                res['top'] = var.token_scores(gt, classes, 'expected_distance', cfg=cfg, top_k=100)
            dist = var.engine().code_distance_table()
            gr = gt.view(2, 1, -1).expand(2, 3, -1).reshape(-1)
            for (score, kw, par), key in zip(D16_CASES, ['group_smoothed', 'neighbor_max', 'expected_distance', 'top']):
                if score == 'neighbor_max':
                    par = d16_kw(var, kw)['threshold']
                want = restate64(z, gr, score, par, dist)
                ok, err = check(res[key].reshape(-1), want, z, score)
                assert ok, f'{prec} cfg={cfg} {score}({par}): max |diff| {err:.3e}'
    finally:
        var.set_hip_precision('f32')


@pytest.mark.parametrize('prec', ['f32', 'bf16'])
def test_packing_is_bitwise_invariant(prec):
    vae, var = d16()
    gt = tokens(var, 3, 13)
    classes = torch.tensor([[4, 90, 1000, 17], [5, 6, 7, 8], [999, 0, 4, 31]], device='cuda')
    perm = torch.tensor([2, 0, 3, 1], device='cuda')
    var.set_hip_precision(prec)
    try:
        for score, kw, _ in D16_CASES:
            kw = d16_kw(var, kw)
            for cfg in (0.0, 1.5):
                u = int(cfg > 0)
                base = var.token_scores(gt, classes, score, cfg=cfg, max_rows=64, **kw)
                for mr in (1 + u, 5):
                    assert torch.equal(var.token_scores(gt, classes, score, cfg=cfg, max_rows=mr, **kw), base), f'{prec} {score} cfg={cfg} max_rows={mr}'
                single = torch.cat([var.token_scores(gt[i:i + 1], classes[i:i + 1], score, cfg=cfg, **kw) for i in range(3)])
                assert torch.equal(single, base), f'{prec} {score} cfg={cfg}: per-image calls differ from the packed call'
                permuted = var.token_scores(gt, classes[:, perm], score, cfg=cfg, **kw)
                assert torch.equal(permuted, base[:, perm]), f'{prec} {score} cfg={cfg}: permuted classes'
    finally:
        var.set_hip_precision('f32')


def test_log_prob_is_token_log_likelihood():
    vae, var = d16()
    gt = tokens(var, 2, 17)
    for cfg in (0.0, 1.5):
        assert torch.equal(var.token_scores(gt, [3, 500, 0], 'log_prob', cfg=cfg), var.token_log_likelihood(gt, [3, 500, 0], cfg=cfg))
    # threshold 0 keeps gt alone (random-init codes are distinct): the same formula and summation order as the log-prob kernel
    cb = var.vae_proxy[0].quantize.embedding.weight
    assert torch.unique(cb, dim=0).shape[0] == var.V
    assert torch.equal(var.token_scores(gt, [3, 500, 0], 'neighbor_max', cfg=1.5, threshold=0.0),
                       var.token_log_likelihood(gt, [3, 500, 0], cfg=1.5))


def test_no_full_logits_tensor():
    """d16, 32 rows per pass (4 images x (7 classes + uncond)): after a warm-up call (which builds the distance table), the peak allocation
    increase of every mode stays below a quarter of R * L * V * 4 bytes, as token_log_likelihood's does"""
    vae, var = d16()
    gt = tokens(var, 4, 4)
    classes = list(range(7))
    full = 32 * var.L * var.V * 4
    for score, kw, _ in D16_CASES:
        kw = d16_kw(var, kw)
        var.token_scores(gt, classes, score, cfg=1.0, max_rows=32, **kw)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        r = var.token_scores(gt, classes, score, cfg=1.0, max_rows=32, **kw)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
        assert r.shape == (4, 7, var.L) and bool(torch.isfinite(r).all())
        assert rise < full / 4, f'{score}: peak allocation rose by {rise / 1e6:.1f} MB (a full logits tensor is {full / 1e6:.0f} MB)'
