"""VAR.patch_effects on the MI355X (d16, three images, ten sites): the clean row is VAR.evaluate bit for bit in every mode, a donor under the
image's own label changes nothing, an attention layer is the group of its heads, zero ablation is weight surgery bit for bit, packings and site
orders give the same bits, the kernel saw the rows the engine meant, no logits tensor is allocated, the 16-bit modes are refused, the calls that
follow find their workspaces as they expect them, and the PyTorch route agrees in all three modes."""
import contextlib
import io

import pytest
import torch

from tests import evalref
from tests import lensref as LR
from tests.test_likelihood_gpu import d16, tokens

pytestmark = pytest.mark.gpu

FIELDS = ('nll', 'entropy', 'kl', 'pred', 'rank')
MODES = ('zero', 'mean', 'donor')
H16 = 16
SITES = (('head', 0, 3), ('head', 7, 15), ('head', 15, 0), ('attn', 0), ('attn', 9), tuple(('head', 9, h) for h in range(H16)), ('mlp', 0), ('mlp', 15),
         (('head', 3, 2), ('mlp', 3)), ('mlp', 8))
ATTN0, ATTN9, HEADS9 = 3, 4, 5
_R = {}


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _inputs():
    vae, var = d16()
    return var, tokens(var, 3, 31), torch.tensor([4, 1000, 31], device='cuda'), torch.tensor([900, 5, 1000], device='cuda')


def _kw(mode, donor=None):
    return dict(mode=mode, donor_label=_inputs()[3] if donor is None else donor) if mode == 'donor' else dict(mode=mode)


def _full(mode):
    """the call on SITES with max_rows 64 (one pass), once per mode; and evaluate"""
    if mode not in _R:
        var, gt, lab, _ = _inputs()
        _R[mode] = var.patch_effects(gt, lab, SITES, **_kw(mode))
        if 'ev' not in _R:
            _R['ev'] = var.evaluate(gt, lab)
    return _R[mode]


def _same(a, i, b, j, what):
    for k in FIELDS:
        assert torch.equal(bits(getattr(a, k)[:, i]), bits(getattr(b, k)[:, j])), f'{what}: {k}'


@pytest.mark.parametrize('mode', MODES)
def test_clean_row_is_evaluate(mode):
    r = _full(mode)
    ev, var = _R['ev'], d16()[1]
    assert r.nll.shape == (3, len(SITES) + 1, var.L) and r.sites[HEADS9] == tuple(('head', 9, h) for h in range(H16)) and r.mode == mode
    assert torch.equal(bits(r.nll[:, 0]), bits(ev.nll_BL)) and torch.equal(r.pred[:, 0], ev.pred_BL) and torch.equal(r.rank[:, 0], ev.rank_BL)
    assert torch.equal(bits(r.kl[:, 0]), torch.zeros(3, var.L, dtype=torch.int32, device='cuda'))
    assert bool(torch.isfinite(r.kl).all()) and bool(torch.isfinite(r.nll).all()) and bool((r.entropy >= 0).all())
    assert bool((r.kl[:, 1:] > 0).any(-1).all()), 'a site whose intervention changes nothing'
    assert r.head_matrix().shape == (16, 16) and int((~torch.isnan(r.head_matrix())).sum()) == 3


def test_donor():
    var, gt, lab, don = _inputs()
    own = var.patch_effects(gt, lab, SITES, mode='donor', donor_label=lab)
    clean = _full('donor')
    for j in range(len(SITES) + 1):
        _same(own, j, clean, 0, f'donor_label == label, row {j}')
    assert bool((clean.kl[:, 1 + ATTN0, 0] > 0).all()), "another label: kl > 0 on the first scale for ('attn', 0)"


@pytest.mark.parametrize('mode', MODES)
def test_site_equivalences(mode):
    var, gt, lab, _ = _inputs()
    r = _full(mode)
    _same(r, 1 + ATTN9, r, 1 + HEADS9, "('attn', 9) against the group of its heads")
    if mode == 'mean':
        first = var.patch_effects(gt, lab, SITES, mode='mean', scales=(0,))
        for j in range(len(SITES) + 1):
            _same(first, j, r, 0, f'mean at scales=(0,), row {j}')


def _model_copy(var):
    """an independent model with var's weights and its VQVAE's: built the way tests.test_likelihood_gpu.d16 builds its own, then loaded"""
    from models import build_vae_var
    with contextlib.redirect_stdout(io.StringIO()):
        vae2, cut = build_vae_var(device='cuda', patch_nums=tuple(var.patch_nums), depth=var.depth, ch=160)
    cut.load_state_dict(var.state_dict())
    vae2.load_state_dict(var.vae_proxy[0].state_dict())
    cut.eval(); vae2.eval(); cut.cond_drop_rate = 0.0
    return cut


def test_zero_ablation_is_weight_surgery():
    """evaluate on a copy of the model whose proj columns / fc2 weight are zeroed: the zero factor adds +-0 to the same fma chain, so the bits of
    nll and pred and rank are those of the ablated row.  This pins the intervention independently of the PyTorch twin."""
    var, gt, lab, _ = _inputs()
    r = _full('zero')
    cut = _model_copy(var)
    for j, site in ((0, ('head', 0, 3)), (1, ('head', 7, 15)), (ATTN9, ('attn', 9)), (7, ('mlp', 15))):
        assert r.sites[j] == (site,)
        blk = cut.blocks[site[1]]
        w = blk.ffn.fc2.weight if site[0] == 'mlp' else blk.attn.proj.weight
        cols = slice(None) if site[0] != 'head' else slice(64 * site[2], 64 * site[2] + 64)
        saved = w.detach()[:, cols].clone()
        with torch.no_grad():
            w[:, cols] = 0
        ev = cut.evaluate(gt, lab)
        with torch.no_grad():
            w[:, cols] = saved
        assert torch.equal(bits(r.nll[:, j + 1]), bits(ev.nll_BL)), f'{site}: nll differs from the weight surgery'
        assert torch.equal(r.pred[:, j + 1], ev.pred_BL) and torch.equal(r.rank[:, j + 1], ev.rank_BL), site
        assert not torch.equal(bits(r.nll[:, j + 1]), bits(r.nll[:, 0]))
    ev = cut.evaluate(gt, lab)                                # the weights are back
    assert torch.equal(bits(ev.nll_BL), bits(_R['ev'].nll_BL))
    del cut


@pytest.mark.parametrize('mode', MODES)
def test_packing_and_site_order_are_bitwise_invariant(mode):
    var, gt, lab, _ = _inputs()
    r = _full(mode)
    least = 3 if mode == 'donor' else 2
    pick = [0, HEADS9, 8, 7] if mode != 'mean' else list(range(len(SITES)))          # (the smallest packing runs a pass per site and image)
    small = var.patch_effects(gt, lab, [SITES[j] for j in pick], max_rows=least, **_kw(mode))
    _same(small, 0, r, 0, f'max_rows={least}: the clean row')
    for i, j in enumerate(pick):
        _same(small, i + 1, r, j + 1, f'max_rows={least}: site {SITES[j]}')
    perm = [9, 2, 5, 0, 7, 4, 8, 1, 6, 3]
    other = var.patch_effects(gt, lab, [SITES[j] for j in perm], max_rows=17, **_kw(mode))          # an image per pass, its sites in one chunk
    for i, j in enumerate(perm):
        _same(other, i + 1, r, j + 1, f'permuted: site {SITES[j]}')
    alone = var.patch_effects(gt[1:2], lab[1:2], SITES[:4], **_kw(mode, _inputs()[3][1:2]))
    for k in FIELDS:
        assert torch.equal(bits(getattr(alone, k)[0]), bits(getattr(r, k)[1, :5])), f'image 1 alone: {k}'


def test_the_kernel_saw_the_right_rows():
    from var_amd.models import args as A
    var, gt, lab, don = _inputs()
    sites = A.patch_sites((SITES[0], SITES[7]), var.depth, var.num_heads)
    cols = A.patch_columns(sites, var.C, 4 * var.C)
    seen = []
    out = var.engine().patch_effects(gt[:1], lab[:1], cols, 'donor', don[:1], tuple(range(len(var.patch_nums))), 64,
                                     _tap=lambda lg, lgc, rows, at: seen.append((lg.cpu(), lgc.cpu(), rows, at)))
    assert [a[3][0] for a in seen] == list(range(len(var.patch_nums)))
    r = _full('donor')
    for lg, lgc, rows, (si, cur, l) in seen:
        assert rows == [(0, -1), (0, 0), (0, 1), (0, 2)]                                 # the donor row, the clean row, the two sites
        V = var.V
        lg, lgc = lg.view(4, l, V), lgc.view(4, l, V)
        assert all(torch.equal(lgc[i], lg[1]) for i in range(4)), 'the gathered rows are not the clean row'
        assert not torch.equal(lg[0], lg[1]) and not torch.equal(lg[2], lg[1])
        want = LR.run_host(lg.reshape(4 * l, V), lgc.reshape(4 * l, V), gt[:1, cur:cur + l].cpu().expand(4, -1).contiguous(), 4, l, V)
        for k, w in zip(FIELDS, want):
            for row, j in ((1, 0), (2, 1), (3, 8)):
                assert torch.equal(bits(out[k][0, row - 1, cur:cur + l]).cpu(), bits(w[row])), (k, si, row)
                assert torch.equal(bits(getattr(r, k)[0, j, cur:cur + l]).cpu(), bits(w[row])), (k, si, row, 'the full call')


def test_no_logits_tensor():
    """d16, 4 images x (clean + 7 sites) = 32 rows in one pass: after a warm-up call the peak allocation rises by the call's own buffers (the
    gathered clean rows of one scale, the per-pass and the returned values, the gathered inputs) and less than a quarter of one (rows, L, V)
    tensor beside them"""
    var = d16()[1]
    gt = tokens(var, 4, 24)
    lab = torch.arange(4, device='cuda')
    var.patch_effects(gt, lab, SITES[:7], mode='zero', max_rows=32)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = var.patch_effects(gt, lab, SITES[:7], mode='zero', max_rows=32)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    R, M = 32, 32 * var.patch_nums[-1] ** 2
    full = R * var.L * var.V * 4
    own = M * var.V * 4 + (R + 4 * 8) * var.L * (4 * 3 + 8 + 4) + R * var.L * (var.Cvae * 4 + 8) + 4 * var.L * (var.Cvae * 4 * 4 + 8 * 2)
    assert r.nll.shape == (4, 8, var.L)
    print(f'peak rise {rise / 1e6:.1f} MB; own buffers {own / 1e6:.1f} MB; one (rows, L, V) tensor {full / 1e6:.1f} MB')
    assert rise < own + full // 4, f'peak allocation rose by {rise / 1e6:.1f} MB'


def test_refused_in_the_16_bit_modes():
    var, gt, lab, _ = _inputs()
    for prec in ('f16', 'bf16'):
        var.set_hip_precision(prec)
        try:
            with pytest.raises(ValueError, match='patch_effects runs in f32'):
                var.patch_effects(gt, lab, SITES[:2])
        finally:
            var.set_hip_precision('f32')


def test_workspaces_left_as_expected():
    var, gt, lab, _ = _inputs()
    _full('zero')
    ev0 = _R['ev']
    img0 = var.autoregressive_infer_cfg(2, lab[:2], g_seed=3, cfg=1.5, top_k=900, top_p=0.96)
    var.patch_effects(gt, lab, SITES[:5], mode='donor', donor_label=7, max_rows=4)
    ev1 = var.evaluate(gt, lab)
    img1 = var.autoregressive_infer_cfg(2, lab[:2], g_seed=3, cfg=1.5, top_k=900, top_p=0.96)
    assert torch.equal(bits(ev1.nll_BL), bits(ev0.nll_BL)) and torch.equal(ev1.pred_BL, ev0.pred_BL) and torch.equal(ev1.rank_BL, ev0.rank_BL)
    assert torch.equal(bits(img1), bits(img0))


@pytest.mark.parametrize('mode', MODES)
def test_pytorch_route_agrees(mode):
    """the same model in train mode (the PyTorch route on the device) against eval mode (the HIP route), f32: nll, entropy and kl at evalref.BAR,
    the bar between the project's two routes; pred on the tokens whose top-2 margin in the PyTorch route's float64 logits exceeds
    2 * evalref.GAP, which must be 90 % of all tokens (checked on the PyTorch route alone, first)."""
    from var_amd.models import args as A
    from var_amd.models.var import patch_effects_torch
    var, gt, lab, don = _inputs()
    a = _full(mode)
    cols = A.patch_columns(a.sites, var.C, 4 * var.C)
    margin = torch.empty(3, len(SITES) + 1, var.L, dtype=torch.float64, device='cuda')

    def tap(n, j, z):
        t2 = z.double().topk(2, dim=-1).values
        margin[n, j] = t2[..., 0] - t2[..., 1]
    var.train()
    try:
        assert not var._scoring_on_hip(var.lvl_1L)
        with torch.no_grad():
            b = dict(zip(FIELDS, patch_effects_torch(var, gt, lab, cols, mode, don if mode == 'donor' else None, a.scales, _tap=tap)))
            pub = var.patch_effects(gt[:1], lab[:1], SITES[:1], **_kw(mode, don[:1]))                # the public call takes the twin here
    finally:
        var.eval()
    assert torch.equal(pub.nll[0], b['nll'][0, :2].float()) and torch.equal(pub.pred[0], b['pred'][0, :2])
    clear = margin > 2 * evalref.GAP
    share = float(clear.double().mean())
    print(f'{mode}: tokens with a top-2 margin above {2 * evalref.GAP}: {share:.4f} (the lowest row: {float(clear.double().mean(-1).min()):.4f})')
    assert share >= 0.9
    worst = {}
    for k in ('nll', 'entropy', 'kl'):
        d = (getattr(a, k).double() - b[k].double()).abs()
        worst[k] = float(d.max())
        print(f'{mode}: {k}: max |HIP - PyTorch| per row {[f"{v:.1e}" for v in d.amax(dim=(0, 2)).tolist()]}')
    for k, v in worst.items():
        assert v <= evalref.BAR, f'{k}: {v:.3e}'
    assert torch.equal(a.pred[clear], b['pred'][clear])
