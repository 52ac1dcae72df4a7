"""VAR.token_log_likelihood on the MI355X: varhip_token_loglik_f32 against float64, the end-to-end API against the reference's logits and
the engine's own teacher-forced logits (d16, every precision, with and without guidance), bitwise packing invariance, and no full logits
tensor in memory."""
import contextlib
import io
import json

import numpy as np
import pytest
import torch

from tests import util
from var_amd import abi, hip

pytestmark = pytest.mark.gpu

PNS16 = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
_M = {}


def kernel_bar_ok(lp, lp64, z):
    """|lp - lp64| <= 1e-6 (|lp64| + max_v |z_v| + 8) per token (a few ulps of the log-sum-exp); z: (..., V) fp32 logits of the rows"""
    zmax = z.abs().amax(-1).double()
    excess = (lp.double() - lp64).abs() - 1e-6 * (lp64.abs() + zmax + 8)
    return float(excess.max()) <= 0, float((lp.double() - lp64).abs().max())


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


def ref_rows(var, vae, gt, classes, cfg):
    """per image: the engine's own teacher-forced logits var(label, x) (one row per class) and, with guidance, the fp32 combine of
    var_analysis.py:333-344 with one unconditional forward -> (N, K, L, V) fp32 z"""
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


@pytest.mark.parametrize('V', [4096, 1000, 4099, 5000])
@pytest.mark.parametrize('cfg', [0.0, 1.5])
def test_kernel_vs_float64(V, cfg):
    """random rows (the pass layout of SamplingEngine.token_log_likelihood) written into a slice of a larger (N, K, L) output"""
    _kernel_vs_float64(V, cfg, (3, 4, 7, 6, 20, 1, 9))


@pytest.mark.parametrize('V', [4096, 4099])
@pytest.mark.parametrize('cfg', [0.0, 1.5])
def test_kernel_vs_float64_slices_end_their_allocations(V, cfg):
    """the same with tok0 + l == L and k0 + classes == K: the last image's tokens are the last elements of gt, its last class row ends the output"""
    _kernel_vs_float64(V, cfg, (3, 4, 7, 6, 16, 2, 9))


def _kernel_vs_float64(V, cfg, layout):
    images, classes, l, K, L, k0, tok0 = layout
    u = 1 if cfg > 0 else 0
    g = torch.Generator(device='cuda').manual_seed(V)
    rows = images * (classes + u) * l
    logits = torch.randn(rows, V, device='cuda', generator=g) * 6
    logits[::5, :7] += 40                                 # a few peaked rows
    gt = torch.randint(0, V, (images, L), device='cuda', generator=g)
    out = torch.full((images, K, L), 12345.0, device='cuda')
    t = np.float32(np.float32(cfg) * np.float32(0.5))
    ca, cb = np.float32(1) + t, t
    util.guarded_call('token_loglik_f32', logits, gt[:, tok0:], L, images, classes, l, V, u, float(ca), float(cb), out[:, k0:, tok0:], K * L, L)
    torch.cuda.synchronize()
    cond = logits[:images * classes * l].view(images, classes, l, V)
    if u:
        unc = logits[images * classes * l:].view(images, 1, l, V)
        z = torch.tensor(ca, device='cuda') * cond - torch.tensor(cb, device='cuda') * unc        # fp32, the kernel's rounding points
    else:
        z = cond
    g_ = gt[:, tok0:tok0 + l].view(images, 1, l, 1).expand(images, classes, l, 1)
    lp64 = z.double().log_softmax(-1).gather(-1, g_).squeeze(-1)
    got = out[:, k0:k0 + classes, tok0:tok0 + l]
    ok, err = kernel_bar_ok(got, lp64, z)
    assert ok, f'V={V} cfg={cfg}: max |lp - lp64| {err:.3e} beyond the bar'
    untouched = torch.ones_like(out, dtype=torch.bool)
    untouched[:, k0:k0 + classes, tok0:tok0 + l] = False
    assert bool((out[untouched] == 12345.0).all()), 'the kernel wrote outside its slice'


def test_kernel_rejects_bad_sizes():
    lg = torch.zeros(64, 256, device='cuda'); gt = torch.zeros(2, 8, dtype=torch.int64, device='cuda'); out = torch.zeros(2, 2, 8, device='cuda')
    f = hip.lib().fn['token_loglik_f32']
    st = hip.current_stream()
    good = [lg.data_ptr(), gt.data_ptr(), 8, 2, 2, 4, 256, 0, 1.0, 0.0, out.data_ptr(), 16, 8]
    assert f(*good, st) == 0
    torch.cuda.synchronize()
    for pos, val in [(3, 0), (4, 0), (5, 0), (6, 0), (2, 3), (12, 3), (11, 8), (0, None)]:
        a = list(good); a[pos] = val
        assert f(*a, st) == abi.EINVAL, (pos, val)


def test_reference_fixture_f32(golden_dir):
    """the d2 fixture (tests/golden/encode_t_pn12345.npz) against the float64 log-softmax-gather of the reference's logits"""
    from models import build_vae_var
    from var_amd.detinit import fill_module_
    z = np.load(f'{golden_dir}/encode_t_pn12345.npz')
    meta = json.loads(str(z['meta']))
    with contextlib.redirect_stdout(io.StringIO()):
        vae, var = build_vae_var(device='cuda', patch_nums=tuple(meta['patch_nums']), depth=meta['depth'], ch=meta['ch'])
    fill_module_(var, meta['depth'], 0, 'var.'); fill_module_(vae, meta['depth'], 0, 'vae.')
    var.eval()
    gt = torch.from_numpy(np.concatenate([z[f'idx_s{si}'] for si in range(len(meta['patch_nums']))], 1).astype(np.int64))
    lp = var.token_log_likelihood(gt.cuda(), torch.tensor(meta['labels']).view(-1, 1))
    ref = torch.from_numpy(z['logits']).double().log_softmax(-1).gather(-1, gt.unsqueeze(-1)).squeeze(-1)
    err = float((lp[:, 0].double().cpu() - ref).abs().max())
    assert err <= 7e-4, f'log p(gt) vs reference logits: {err:.3e}'


@pytest.mark.parametrize('prec', ['f32', 'f16', 'bf16', 'auto'])
def test_d16_vs_engine_logits(prec):
    """L = 680: against the float64 log-softmax of the engine's own teacher-forced logits, same precision"""
    vae, var = d16()
    gt = tokens(var, 2, 1)
    classes = [1, 207, 999]
    ctx = torch.autocast('cuda', dtype=torch.bfloat16) if prec == 'auto' else contextlib.nullcontext()
    var.set_hip_precision(prec)
    try:
        with torch.no_grad(), ctx:
            lp = var.token_log_likelihood(gt, classes)
            z = ref_rows(var, vae, gt, classes, 0.0)
            if prec == 'auto':
                assert var.engine().precision == 'bf16'
    finally:
        var.set_hip_precision('f32')
    lp64 = z.double().log_softmax(-1).gather(-1, gt.view(2, 1, -1, 1).expand(2, 3, -1, 1)).squeeze(-1)
    ok, err = kernel_bar_ok(lp, lp64, z)
    assert ok, f'{prec}: max |lp - lp64| {err:.3e}'


@pytest.mark.parametrize('prec', ['f32', 'bf16'])
def test_d16_cfg_vs_engine_logits(prec):
    vae, var = d16()
    gt = tokens(var, 2, 2)
    classes, cfg = [3, 500, 0, 998], 1.5
    var.set_hip_precision(prec)
    try:
        with torch.no_grad():
            lp = var.token_log_likelihood(gt, classes, cfg=cfg)
            z = ref_rows(var, vae, gt, classes, cfg)
    finally:
        var.set_hip_precision('f32')
    lp64 = z.double().log_softmax(-1).gather(-1, gt.view(2, 1, -1, 1).expand(2, 4, -1, 1)).squeeze(-1)
    ok, err = kernel_bar_ok(lp, lp64, z)
    assert ok, f'{prec} cfg: max |lp - lp64| {err:.3e}'


@pytest.mark.parametrize('prec', ['f32', 'f16', 'bf16'])
def test_packing_is_bitwise_invariant(prec):
    vae, var = d16()
    gt = tokens(var, 3, 3)
    classes = torch.tensor([[4, 90, 1000, 17], [5, 6, 7, 8], [999, 0, 4, 31]], device='cuda')
    perm = torch.tensor([2, 0, 3, 1], device='cuda')
    var.set_hip_precision(prec)
    try:
        for cfg in (0.0, 2.0):
            u = int(cfg > 0)
            base = var.token_log_likelihood(gt, classes, cfg=cfg, max_rows=64)
            for mr in (1 + u, 5):
                assert torch.equal(var.token_log_likelihood(gt, classes, cfg=cfg, max_rows=mr), base), f'{prec} cfg={cfg} max_rows={mr}'
            single = torch.cat([var.token_log_likelihood(gt[i:i + 1], classes[i:i + 1], cfg=cfg) for i in range(3)])
            assert torch.equal(single, base), f'{prec} cfg={cfg}: per-image calls differ from the packed call'
            permuted = var.token_log_likelihood(gt, classes[:, perm], cfg=cfg)
            assert torch.equal(permuted, base[:, perm]), f'{prec} cfg={cfg}: permuted classes'
    finally:
        var.set_hip_precision('f32')


def test_no_full_logits_tensor():
    """d16, 32 rows per pass (4 images x (7 classes + uncond)): after a warm-up call, the second call's peak allocation increase stays below a
    quarter of R * L * V * 4 bytes"""
    vae, var = d16()
    gt = tokens(var, 4, 4)
    classes = list(range(7))
    var.token_log_likelihood(gt, classes, cfg=1.0, max_rows=32)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    lp = var.token_log_likelihood(gt, classes, cfg=1.0, max_rows=32)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    full = 32 * var.L * var.V * 4
    assert lp.shape == (4, 7, var.L) and bool(torch.isfinite(lp).all())
    assert rise < full / 4, f'peak allocation rose by {rise / 1e6:.1f} MB (a full logits tensor is {full / 1e6:.0f} MB)'
