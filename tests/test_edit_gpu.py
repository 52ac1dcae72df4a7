"""VAR.autoregressive_infer_cfg_with_mask on a real MI355X (zero-shot editing, demo_zero_shot_edit.ipynb cell 2):
  - varhip_edit_keep_u8 against F.interpolate(...) > 0.5 computed by torch on the CPU and on this GPU, and the reference's recorded maps;
  - the fused quantizer steps bitwise against token_select_i64 + quant_accum_f32 and an overwrite of h + quant_accum_h_f32;
  - the reference fixtures (tools/gen_golden_edit.py) with their own Exp(1) / gumbel streams injected: tokens identical, f_hat and image within
    the inpainting tests' tolerances;
  - identities (no mask == plain sampling, all-ones mask == idxBl_to_img of the input and the same RNG state, one row == its repeat);
  - the 16-bit modes."""
import json

import numpy as np
import pytest

from tests import util
from tests.test_e2e_gpu import build_models

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
F = pytest.importorskip('torch.nn.functional')

EDIT_FIXTURES = ['a_inpaint', 'b_outpaint', 'c_b3_7x9', 'd_more_smooth', 'e_saln', 'f_half']
PUBLISHED = [(1, 2, 3, 4, 5, 6, 8, 10, 13, 16), (1, 2, 3, 4, 6, 9, 13, 18, 24, 32)]
FIXTURE_PNS = [(1, 2, 3, 4, 5), (1, 2, 3, 4, 6)]


def keep_kernel(mask, pns, B):
    """(B, L) uint8 keep map from varhip_edit_keep_u8; mask (Bm, h, w) fp32 on the GPU"""
    from var_amd import hip
    L = sum(p * p for p in pns)
    out = torch.full((B, L), 7, dtype=torch.uint8, device='cuda')
    util.guarded_call('edit_keep_u8', mask, mask.shape[0], mask.shape[1], mask.shape[2], torch.tensor(pns, dtype=torch.int32), len(pns), B, out)
    return out


def keep_torch(mask, pns, B):
    """the rule of replace_embedding, evaluated by torch on the mask's device"""
    m = mask.expand(B, -1, -1) if mask.shape[0] == 1 else mask
    ks = []
    for pn in pns:
        k = F.interpolate(m[:, None].float(), size=(pn, pn), mode='bilinear', align_corners=False) > 0.5
        if pn * pn <= 3: k = torch.ones_like(k)
        ks.append(k.reshape(B, -1))
    return torch.cat(ks, 1).to(torch.uint8)


def edit_box(pns, y0, x0, y1, x1, inpainting):
    from models.var import get_edit_mask
    return get_edit_mask(pns, y0, x0, y1, x1, 'cuda', inpainting=inpainting)


def binary_masks(P):
    g = torch.Generator().manual_seed(P)
    out = []
    corners = [0.0, 0.1, 0.25, 0.3, 0.5, 0.55, 0.8, 1.0]
    for y0 in corners[:4]:
        for x0 in corners[:4]:
            for y1 in corners[4:]:
                for x1 in corners[4:]:
                    out.append(edit_box((P,), y0, x0, y1, x1, True)[None])
                    out.append(edit_box((P,), y0, x0, y1, x1, False)[None])
    for h, w in ((1, 1), (7, 9), (P, P), (512, 512)):
        out.append((torch.rand(3, h, w, generator=g) < 0.5).float().cuda())
        out.append(torch.ones(1, h, w, device='cuda'))
        out.append(torch.zeros(1, h, w, device='cuda'))
    return out


@pytest.mark.parametrize('pns', FIXTURE_PNS + PUBLISHED)
def test_keep_kernel_equals_interpolate_on_binary_masks(pns):
    """get_edit_mask boxes over a grid of corners (in- and out-painting) and random binary masks of 1x1, 7x9, PxP and 512x512: the kernel's
    map equals F.interpolate(...) > 0.5 computed by torch on the CPU and on this GPU, bit for bit"""
    P = pns[-1]
    bad_cpu = bad_gpu = 0
    n = 0
    for m in binary_masks(P):
        B = 3 if m.shape[0] == 3 else 2
        got = keep_kernel(m, pns, B)
        assert int(got.max()) <= 1
        cpu = keep_torch(m.cpu(), pns, B)
        gpu = keep_torch(m, pns, B).cpu()
        n += 1
        bad_cpu += int(not torch.equal(got.cpu(), cpu))
        bad_gpu += int(not torch.equal(got.cpu(), gpu))
    print(f'pns {pns}: {n} binary masks, kernel != torch CPU on {bad_cpu}, kernel != torch GPU on {bad_gpu}')
    assert bad_cpu == 0
    assert bad_gpu == 0


@pytest.mark.parametrize('pns', FIXTURE_PNS + PUBLISHED)
def test_keep_kernel_on_real_masks(pns):
    """random real-valued masks (uniform, and concentrated within 1e-3 of 1/2 where the blend's rounding decides): the kernel against torch
    on the CPU and on this GPU: equal to torch on this GPU everywhere, and to torch on the CPU wherever torch's two builds agree with each other
    (they disagree at a few near-1/2 positions)"""
    P = pns[-1]
    g = torch.Generator().manual_seed(100 + P)
    stats = dict(n=0, cpu=0, gpu=0, cpu_vs_gpu=0)
    for h, w in ((1, 1), (7, 9), (P, P), (512, 512)):
        for near in (False, True):
            m = torch.rand(3, h, w, generator=g)
            if near: m = 0.5 + (m - 0.5) * 1e-3
            m = m.cuda()
            got = keep_kernel(m, pns, 3).cpu()
            cpu = keep_torch(m.cpu(), pns, 3)
            gpu = keep_torch(m, pns, 3).cpu()
            stats['n'] += got.numel()
            stats['cpu'] += int((got != cpu).sum()); stats['gpu'] += int((got != gpu).sum()); stats['cpu_vs_gpu'] += int((cpu != gpu).sum())
            stats['cpu_where_torch_agrees'] = stats.get('cpu_where_torch_agrees', 0) + int(((got != cpu) & (cpu == gpu)).sum())
    print(f'pns {pns}: real masks, {stats}')
    assert stats['gpu'] == 0 and stats['cpu_where_torch_agrees'] == 0


@pytest.mark.parametrize('name', EDIT_FIXTURES)
def test_keep_kernel_equals_the_reference_maps(name, golden_dir):
    z = np.load(f'{golden_dir}/edit_{name}.npz')
    meta = json.loads(str(z['meta']))
    got = keep_kernel(torch.from_numpy(z['mask']).cuda(), meta['patch_nums'], meta['B']).cpu().numpy()
    assert np.array_equal(got, z['keep'])


def test_keep_kernel_rejects_bad_sizes():
    from var_amd import hip
    m = torch.ones(2, 4, 4, device='cuda')
    out = torch.empty(3, 55, dtype=torch.uint8, device='cuda')
    with pytest.raises(hip.VarHipError):
        hip.call('edit_keep_u8', m, 2, 4, 4, torch.tensor([1, 2, 3, 4, 5], dtype=torch.int32), 5, 3, out)     # Bm neither 1 nor B
    with pytest.raises(hip.VarHipError):
        hip.call('edit_keep_u8', m, 1, 0, 4, torch.tensor([1, 2, 3, 4, 5], dtype=torch.int32), 5, 3, out)


@pytest.mark.parametrize('pn', [1, 3, 4, 5])
@pytest.mark.parametrize('smooth', [False, True])
def test_fused_quantizer_step_equals_select_then_step(pn, smooth):
    _fused_step_case(pn, smooth, at_end=False)


@pytest.mark.parametrize('pn', [1, 3, 4, 5])
@pytest.mark.parametrize('smooth', [False, True])
def test_fused_quantizer_step_with_keep_and_gt_ending_their_rows(pn, smooth):
    """the scale's l tokens are the LAST l columns of the (B, ld) keep / gt rows: the last row's last element ends both allocations"""
    _fused_step_case(pn, smooth, at_end=True)


def _fused_step_case(pn, smooth, at_end):
    from var_amd import hip
    from var_amd.engine import phi_index
    meta = dict(depth=2, ch=32, patch_nums=(1, 2, 3, 4, 5), attn_l2_norm=True, shared_aln=False)
    vae, var = build_models(meta)
    eng = var.engine(); eng.refresh(); eng._wait_ready()
    w = eng.w
    B, P, Cv, V, S = 3, 5, var.Cvae, var.V, 5
    l, ld = pn * pn, var.L + 7
    off = ld - l if at_end else 11
    g = torch.Generator(device='cuda').manual_seed(pn)
    idx = torch.randint(0, V, (B * l,), device='cuda', generator=g)
    gt = torch.randint(0, V, (B, ld), device='cuda', generator=g)
    keep = (torch.rand(B, ld, device='cuda', generator=g) < 0.5).to(torch.uint8)
    ti, tw = w['taps'].get(pn, (None, None))
    pw, pb, ratio = w['phi'][phi_index(var.patch_nums.index(pn), S, len(w['phi']))]
    f0 = torch.randn(B, P, P, Cv, device='cuda', generator=g)
    up_a, up_b = torch.empty_like(f0), torch.empty_like(f0)
    fa, fb = f0.clone(), f0.clone()
    ks, gs = keep[:, off:off + l].contiguous(), gt[:, off:off + l].contiguous()
    if not smooth:
        sel = torch.empty_like(idx)
        util.guarded_call('token_select_i64', ks, gs, idx, sel, B * l)
        util.guarded_call('quant_accum_f32', sel, w['codebook'], ti, tw, pw, pb, ratio, up_a, fa, B, pn, P, Cv)
        util.guarded_call('quant_accum_edit_f32', idx, keep[:, off:], gt[:, off:], ld, w['codebook'], ti, tw, pw, pb, ratio, up_b, fb, B, pn, P, Cv)
    else:
        h = torch.randn(B * l, Cv, device='cuda', generator=g)
        h2 = h.clone().view(B, l, Cv)
        h2[ks.bool()] = w['codebook'][gs[ks.bool()]]
        util.guarded_call('quant_accum_h_f32', h2, ti, tw, pw, pb, ratio, up_a, fa, B, pn, P, Cv)
        util.guarded_call('quant_accum_h_edit_f32', h, keep[:, off:], gt[:, off:], ld, w['codebook'], ti, tw, pw, pb, ratio, up_b, fb, B, pn, P, Cv)
    torch.cuda.synchronize()
    assert torch.equal(up_a, up_b) and torch.equal(fa, fb)


def regen_edit_noise(meta, z):
    """the fills the notebook's loop consumed: per scale one (B*l, V) Exp(1) fill, then with more_smooth the (B, l, V) gumbel one"""
    g = torch.Generator(); g.manual_seed(meta['seed'])
    n1, n2 = [], []
    for si, pn in enumerate(meta['patch_nums']):
        a = torch.empty(meta['B'] * pn * pn, meta['V']).exponential_(1, generator=g)
        if meta['more_smooth']:
            b = torch.empty(meta['B'] * pn * pn, meta['V']).exponential_(generator=g)
            head = np.concatenate([a.view(-1)[:4].numpy(), b.view(-1)[:4].numpy()])
            n2.append(b)
        else:
            head = a.view(-1)[:8].numpy()
        assert np.array_equal(head, z['noise_head'][si])
        n1.append(a)
    return n1, (n2 if meta['more_smooth'] else None)


def run_fixture(meta, z, force=None):
    vae, var = build_models(meta)
    n1, n2 = regen_edit_noise(meta, z)
    B = meta['B']
    labels = torch.tensor(meta['labels'], device='cuda')
    toks = torch.from_numpy(z['tokens'].astype(np.int64)).cuda()
    out = torch.empty(B, var.L, dtype=torch.int64, device='cuda')
    eng = var.engine()
    img = eng.sample(B, labels, None, meta['cfg'], meta['top_k'], meta['top_p'], noises=n1, gumbel_noises=n2, more_smooth=meta['more_smooth'],
                     trace=True, tokens_out=out, force_idx=force, edit=dict(tokens=toks, mask=torch.from_numpy(z['mask']).cuda()))
    torch.cuda.synchronize()
    return img, out, eng.last_trace


@pytest.mark.parametrize('name', EDIT_FIXTURES)
def test_edit_vs_reference(name, golden_dir):
    z = np.load(f'{golden_dir}/edit_{name}.npz')
    meta = json.loads(str(z['meta']))
    vae, var = build_models(meta)
    var.set_hip_precision('f32')
    img, out, tr = run_fixture(meta, z)
    out = out.cpu().numpy()
    keep = z['keep'].astype(bool)
    assert np.array_equal(out[keep], z['tokens'][keep])
    ok, m = util.diff_report(f'{name} final tokens vs reference', out.astype(np.int32), z['final']); print(m); assert ok, m
    cur = 0
    for si, pn in enumerate(meta['patch_nums']):
        l = pn * pn
        if tr['sampled'][si] is not None:
            ok, m = util.diff_report(f'{name} sampled tokens s{si}', tr['sampled'][si].cpu().numpy().astype(np.int32), z['sampled'][:, cur:cur + l])
            assert ok, m
        else:
            assert keep[:, cur:cur + l].all()
        cur += l
    # more_smooth: the gumbel softmax at tau = 0.0135 amplifies logit rounding (tests/test_oracle_vs_golden.py::test_more_smooth_case), so
    # f_hat takes the image's 2e-3 there
    ftol = 2e-3 if meta['more_smooth'] else 2e-5
    ok, m = util.diff_report(f'{name} f_hat vs reference', tr['f_hat'][-1].cpu().numpy(), z['f_hat'], atol=ftol, rtol=1e-5); print(m); assert ok, m
    tol = 2e-3 if meta['more_smooth'] else 1e-4
    ok, m = util.diff_report(f'{name} image vs reference', img.cpu().numpy(), z['img'], atol=tol); print(m); assert ok, m


def _scales(t, pns):
    out, cur = [], 0
    for pn in pns:
        out.append(t[:, cur:cur + pn * pn]); cur += pn * pn
    return out


def test_identities(golden_dir):
    z = np.load(f'{golden_dir}/edit_a_inpaint.npz')
    meta = json.loads(str(z['meta']))
    vae, var = build_models(meta)
    var.set_hip_precision('f32')
    B, pns = meta['B'], meta['patch_nums']
    toks = torch.from_numpy(z['tokens'].astype(np.int64)).cuda()
    labels = torch.tensor(meta['labels'], device='cuda')
    kw = dict(cfg=1.5, top_k=900, top_p=0.96)
    # no mask: the plain call, bit for bit
    a = var.autoregressive_infer_cfg_with_mask(B, labels, g_seed=7, **kw).clone()
    b = var.autoregressive_infer_cfg(B, labels, g_seed=7, **kw).clone()
    assert torch.equal(a, b)
    # all-ones mask: the decode of the input tokens, and the generator where a plain call leaves it
    full = var.autoregressive_infer_cfg_with_mask(B, labels, g_seed=7, input_img_tokens=_scales(toks, pns), edit_mask=torch.ones(9, 9), **kw).clone()
    nxt_edit = torch.empty(4096, device='cuda').exponential_(generator=var.rng)
    var.autoregressive_infer_cfg(B, labels, g_seed=7, **kw)
    nxt_plain = torch.empty(4096, device='cuda').exponential_(generator=var.rng)
    assert torch.equal(nxt_edit, nxt_plain)
    with torch.inference_mode():
        ref = vae.idxBl_to_img(_scales(toks, pns), same_shape=True, last_one=True).add_(1).mul_(0.5)
    ok, m = util.diff_report('all-ones mask == idxBl_to_img (exact)', full.cpu().numpy(), ref.cpu().numpy()); print(m); assert ok, m
    # more_smooth with the same mask: the same generator state too
    var.autoregressive_infer_cfg_with_mask(B, labels, g_seed=7, input_img_tokens=toks, edit_mask=torch.ones(5, 5), more_smooth=True, **kw)
    nxt_edit = torch.empty(4096, device='cuda').exponential_(generator=var.rng)
    var.autoregressive_infer_cfg(B, labels, g_seed=7, more_smooth=True, **kw)
    assert torch.equal(nxt_edit, torch.empty(4096, device='cuda').exponential_(generator=var.rng))
    # one row broadcasts: equal to its B-row repeat; the concatenated form equals the per-scale list
    mask = torch.from_numpy(z['mask'][0])
    one = var.autoregressive_infer_cfg_with_mask(B, labels, g_seed=9, input_img_tokens=toks[:1], edit_mask=mask, **kw).clone()
    rep = var.autoregressive_infer_cfg_with_mask(B, labels, g_seed=9, input_img_tokens=_scales(toks[:1].repeat(B, 1), pns), edit_mask=mask, **kw).clone()
    assert torch.equal(one, rep)
    bm = var.autoregressive_infer_cfg_with_mask(B, labels, g_seed=9, input_img_tokens=toks[:1], edit_mask=mask[None].expand(B, -1, -1).bool(), **kw)
    assert torch.equal(one, bm)
    # the public call on the fixture's tokens keeps them: decode of its f_hat path is deterministic
    c = var.autoregressive_infer_cfg_with_mask(B, labels, g_seed=9, input_img_tokens=toks, edit_mask=mask, **kw).clone()
    d = var.autoregressive_infer_cfg_with_mask(B, labels, g_seed=9, input_img_tokens=toks, edit_mask=mask, **kw)
    assert torch.equal(c, d) and c.shape == (B, 3, 80, 80)
    with pytest.raises(ValueError):
        var.engine().sample(B, labels, None, 1.5, 900, 0.96, edit=dict(tokens=toks, mask=mask[None].cuda()), greedy=True)


@pytest.mark.parametrize('name', ['a_inpaint', 'c_b3_7x9', 'd_more_smooth', 'e_saln', 'f_half'])
@pytest.mark.parametrize('mode', ['f16', 'bf16', 'auto_f16', 'auto_bf16'])
def test_edit_16bit(name, mode, golden_dir):
    """16-bit transformer: kept tokens exactly the input, images finite and in [0, 1]; with the reference's final tokens forced, pixels within
    the bars of the end-to-end tests: f16 2e-2 (tests/test_f16_gpu.py), bf16 max 1.6e-1 and mean 1.6e-2 (tests/test_bf16_gpu.py); keep maps
    and the quantizer step stay fp32"""
    import contextlib
    z = np.load(f'{golden_dir}/edit_{name}.npz')
    meta = json.loads(str(z['meta']))
    vae, var = build_models(meta)
    flav = mode.split('_')[-1]
    var.set_hip_precision('auto' if mode.startswith('auto') else flav)
    ctx = torch.autocast('cuda', dtype=torch.float16 if flav == 'f16' else torch.bfloat16) if mode.startswith('auto') else contextlib.nullcontext()
    try:
        with ctx:
            img, out, tr = run_fixture(meta, z)
            keep = z['keep'].astype(bool)
            assert np.array_equal(out.cpu().numpy()[keep], z['tokens'][keep])
            assert torch.isfinite(img).all() and float(img.min()) >= 0 and float(img.max()) <= 1
            assert var.engine().precision == flav
            if not meta['more_smooth']:
                img_f, _, _ = run_fixture(meta, z, force=torch.from_numpy(z['final'].astype(np.int64)))
                d = np.abs(img_f.cpu().numpy() - z['img'])
                print(f'{name} {mode} image (reference tokens forced) vs reference: max |d| {float(d.max()):.3e} mean {float(d.mean()):.2e}')
                if flav == 'f16':
                    assert float(d.max()) <= 2e-2
                else:
                    assert float(d.max()) <= 1.6e-1 and float(d.mean()) <= 1.6e-2
            lab = torch.tensor(meta['labels'], device='cuda')
            pub = var.autoregressive_infer_cfg_with_mask(meta['B'], lab, g_seed=1, input_img_tokens=torch.from_numpy(z['tokens'].astype(np.int64)),
                                                         edit_mask=torch.from_numpy(z['mask']), more_smooth=meta['more_smooth'])
            assert torch.isfinite(pub).all() and float(pub.min()) >= 0 and float(pub.max()) <= 1
    finally:
        var.set_hip_precision('f32')
