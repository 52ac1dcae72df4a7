"""VAR.logit_lens on the MI355X (d16, three images): the last layer is VAR.evaluate bit for bit, the kernel saw the rows the engine meant (host
twin on tapped clones), layer subsets and packings are the same bits, no per-layer logits tensor is allocated, the PyTorch route agrees, and the
calls that follow find their workspaces as they expect them."""
import numpy as np
import pytest
import torch

from tests import evalref
from tests import lensref as LR
from tests.test_likelihood_gpu import d16, tokens

pytestmark = pytest.mark.gpu

FIELDS = ('nll', 'entropy', 'kl', 'pred', 'rank')
_R = {}


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _inputs():
    vae, var = d16()
    return var, tokens(var, 3, 31), torch.tensor([4, 1000, 31], device='cuda')


def _full(prec='f32'):
    """the full call (all layers, max_rows 64), once per precision"""
    if prec not in _R:
        var, gt, lab = _inputs()
        var.set_hip_precision(prec)
        try:
            _R[prec] = (var.logit_lens(gt, lab), var.evaluate(gt, lab))
        finally:
            var.set_hip_precision('f32')
    return _R[prec]


def _same(a, b, what, sl=slice(None)):
    for k in FIELDS:
        assert torch.equal(bits(getattr(a, k)), bits(getattr(b, k)[:, sl])), f'{what}: {k}'


@pytest.mark.parametrize('prec', ['f32', 'bf16'])
def test_last_layer_is_evaluate(prec):
    r, ev = _full(prec)
    var = d16()[1]
    assert r.nll.shape == (3, var.depth, var.L) and r.layers == tuple(range(var.depth))
    assert torch.equal(bits(r.nll[:, -1]), bits(ev.nll_BL)) and torch.equal(r.pred[:, -1], ev.pred_BL) and torch.equal(r.rank[:, -1], ev.rank_BL)
    assert torch.equal(bits(r.kl[:, -1]), torch.zeros(3, var.L, dtype=torch.int32, device='cuda'))
    assert bool(torch.isfinite(r.kl).all()) and bool((r.entropy >= 0).all()) and bool((r.entropy <= float(np.log(var.V)) * (1 + 1e-6)).all())
    assert bool((r.kl[:, 0] > 0).all())


def test_the_kernel_saw_the_right_rows():
    var, gt, lab = _inputs()
    seen = []
    var.engine().logit_lens(gt[:2], lab[:2], (3, 15), 64, _tap=lambda lg, lgf, at: seen.append((lg.cpu(), lgf.cpu(), at)))
    S = len(var.patch_nums)
    assert [a[2][:2] for a in seen] == [(bi, si) for si in range(S) for bi in (3, 15)]
    r = _full()[0]
    for lg, lgf, (bi, si, cur, l) in seen:
        want = LR.run_host(lg, lgf, gt[:2, cur:cur + l].cpu().contiguous(), 2, l, var.V)
        assert torch.equal(lg, lgf) == (bi == 15)
        for k, w in zip(FIELDS, want):
            assert torch.equal(bits(getattr(r, k)[:2, bi, cur:cur + l]).cpu(), bits(w)), (k, bi, si)


def test_layer_subsets_are_slices_of_the_full_call():
    var, gt, lab = _inputs()
    r = _full()[0]
    sub = var.logit_lens(gt, lab, layers=(0, 7, 15))
    _same(sub, r, 'layers (0, 7, 15)', [0, 7, 15])
    _same(var.logit_lens(gt, lab, layers=(2,)), r, 'layers (2,)', [2])


@pytest.mark.parametrize('prec', ['f32', 'bf16'])
def test_packing_is_bitwise_invariant(prec):
    var, gt, lab = _inputs()
    r = _full(prec)[0]
    var.set_hip_precision(prec)
    try:
        for mr in (1, 2):
            _same(var.logit_lens(gt, lab, layers=(0, 9, 15), max_rows=mr), r, f'{prec} max_rows={mr}', [0, 9, 15])
        alone = var.logit_lens(gt[1:2], lab[1:2], layers=(0, 9, 15))
    finally:
        var.set_hip_precision('f32')
    for k in FIELDS:
        assert torch.equal(bits(getattr(alone, k)[0]), bits(getattr(r, k)[1, [0, 9, 15]])), f'{prec} image 1 alone: {k}'


def test_no_per_layer_logits_tensor():
    """d16, 8 images in one pass, all layers: after a warm-up call the peak allocation rises by less than one (N, L, V) tensor plus the call's own
    buffers (the stash, lg2) and its outputs; the route through hooks holds depth such tensors"""
    var = d16()[1]
    gt = tokens(var, 8, 24)
    lab = torch.arange(8, device='cuda')
    var.logit_lens(gt, lab, max_rows=8)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = var.logit_lens(gt, lab, max_rows=8)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    M = 8 * var.patch_nums[-1] ** 2
    full = 8 * var.L * var.V * 4
    own = (var.depth - 1) * M * var.C * 4 + M * var.V * 4 + 8 * var.depth * var.L * (4 * 4 + 8)
    xin = 8 * var.L * (var.Cvae * 4 * 4 + 8 * 2)                 # the teacher-forcing input and its temporaries
    assert r.nll.shape == (8, var.depth, var.L)
    print(f'peak rise {rise / 1e6:.1f} MB; stash + lg2 + outputs {own / 1e6:.1f} MB; one logits tensor {full / 1e6:.1f} MB')
    assert rise < full + own + xin, f'peak allocation rose by {rise / 1e6:.1f} MB'


def test_pytorch_route_agrees():
    """the same model in train mode (the PyTorch route on the device, drop path off) against eval mode (the HIP route), f32: nll, entropy and kl
    at evalref.BAR, the bar tests/test_evaluate_gpu.py holds nll to between its two routes; pred on the tokens whose top-2 margin in the PyTorch
    route's float64 logits exceeds 2 * evalref.GAP (GAP: what two logits may move by between the routes), which must be 90 % of all tokens"""
    from var_amd.models.helpers import DropPath
    var, gt, lab = _inputs()
    a = _full()[0]
    saved = [(m, m.drop_prob) for m in var.modules() if isinstance(m, DropPath)]
    for m, _ in saved:
        m.drop_prob = 0.0
    var.train()
    try:
        assert not var._scoring_on_hip(var.lvl_1L)
        with torch.no_grad():
            b = var.logit_lens(gt, lab, max_rows=1)
            caught = {}
            hooks = [blk.register_forward_hook(lambda mod, inp, out, bi=bi: caught.__setitem__(bi, out)) for bi, blk in enumerate(var.blocks)]
            x = var.vae_proxy[0].quantize.idxBl_to_var_input([gt[:, s:e] for s, e in var.begin_ends])
            var._forward_torch(lab, x)
            for h in hooks:
                h.remove()
            cond = var.class_emb(lab)
            margin = []
            for bi in range(var.depth):
                t2 = var.get_logits(caught[bi].float(), cond).double().topk(2, dim=-1).values
                margin.append(t2[..., 0] - t2[..., 1])
            margin = torch.stack(margin, 1)
    finally:
        var.eval()
        for m, p in saved:
            m.drop_prob = p
    for k in ('nll', 'entropy', 'kl'):
        d = (getattr(a, k).double() - getattr(b, k).double()).abs()
        print(f'{k}: max |HIP - PyTorch| per layer {[f"{v:.1e}" for v in d.amax(dim=(0, 2)).tolist()]}')
    clear = margin > 2 * evalref.GAP
    share = float(clear.double().mean())
    print(f'tokens with a top-2 margin above {2 * evalref.GAP}: {share:.4f}')
    for k in ('nll', 'entropy', 'kl'):
        d = (getattr(a, k).double() - getattr(b, k).double()).abs()
        assert float(d.max()) <= evalref.BAR, f'{k}: {float(d.max()):.3e}'
    assert share >= 0.9 and torch.equal(a.pred[clear], b.pred[clear])


def test_workspaces_left_as_expected():
    var, gt, lab = _inputs()
    ev0 = _full()[1]
    img0 = var.autoregressive_infer_cfg(2, lab[:2], g_seed=3, cfg=1.5, top_k=900, top_p=0.96)
    var.logit_lens(gt, lab, layers=(5, 15), max_rows=2)
    ev1 = var.evaluate(gt, lab)
    img1 = var.autoregressive_infer_cfg(2, lab[:2], g_seed=3, cfg=1.5, top_k=900, top_p=0.96)
    assert torch.equal(bits(ev1.nll_BL), bits(ev0.nll_BL)) and torch.equal(ev1.pred_BL, ev0.pred_BL) and torch.equal(ev1.rank_BL, ev0.rank_BL)
    assert torch.equal(bits(img1), bits(img0))
