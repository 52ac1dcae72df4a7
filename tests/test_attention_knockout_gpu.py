"""VAR.attention_knockout on the MI355X (d16, two images, eleven entries with a tuple, a per-layer and a per-head edge): the clean row is
VAR.evaluate bit for bit, the scales below a cut are untouched, an edge over all layers is the tuple of its per-layer edges, packings and entry
orders give the same bits, no logits tensor is allocated, the 16-bit modes are refused, and the PyTorch route agrees."""
import pytest
import torch

from tests import evalref
from tests.test_likelihood_gpu import d16, tokens

pytestmark = pytest.mark.gpu

FIELDS = ('nll', 'entropy', 'kl', 'pred', 'rank')
DEPTH = 16
EDGES = ((1, 0), (4, 4), (6, 2), (9, 8), (9, 0), (7, 7), ((5, 0), (5, 1), (5, 2)), (8, 3, 5), (6, 5, 9, 3), (3, 1), tuple((3, 1, b) for b in range(DEPTH)))
WHOLE31, LAYERS31 = 9, 10
_R = {}


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _inputs():
    vae, var = d16()
    return var, tokens(var, 2, 47), torch.tensor([4, 1000], device='cuda')


def _full():
    """the call on EDGES with max_rows 64 (one pass), once; and evaluate"""
    if 'r' not in _R:
        var, gt, lab = _inputs()
        _R['r'] = var.attention_knockout(gt, lab, EDGES)
        _R['ev'] = var.evaluate(gt, lab)
    return _R['r']


def _same(a, i, b, j, what, tok=slice(None)):
    for k in FIELDS:
        assert torch.equal(bits(getattr(a, k)[:, i, tok]), bits(getattr(b, k)[:, j, tok])), f'{what}: {k}'


def test_clean_row_is_evaluate():
    r = _full()
    ev, var = _R['ev'], d16()[1]
    assert r.nll.shape == (2, len(EDGES) + 1, var.L) and r.edges[7] == ((8, 3, (5,), tuple(range(16))),) and r.edges[8] == ((6, 5, (9,), (3,)),)
    assert torch.equal(bits(r.nll[:, 0]), bits(ev.nll_BL)) and torch.equal(r.pred[:, 0], ev.pred_BL) and torch.equal(r.rank[:, 0], ev.rank_BL)
    assert torch.equal(bits(r.kl[:, 0]), torch.zeros(2, var.L, dtype=torch.int32, device='cuda'))
    assert bool(torch.isfinite(r.kl).all()) and bool(torch.isfinite(r.nll).all()) and bool((r.entropy >= 0).all())
    m = r.edge_matrix()
    assert m.shape == (10, 10) and int((~torch.isnan(m)).sum()) == 9 and bool(torch.isfinite(r.edge_matrix(at='all')[9, 0]))


def test_causality_and_the_all_layers_identity():
    var = d16()[1]
    r = _full()
    for j, group in enumerate(r.edges):
        q0 = min(e[0] for e in group)
        b, e = var.begin_ends[q0]
        _same(r, j + 1, r, 0, f'{EDGES[j]}: the scales below {q0}', slice(0, b))
        assert bool((r.kl[:, j + 1, b:e] > 0).any(-1).all()), f'{EDGES[j]}: no token of scale {q0} changed'
    _same(r, 1 + WHOLE31, r, 1 + LAYERS31, '(3, 1) over all layers against the tuple of its per-layer edges')


def test_packing_and_entry_order_are_bitwise_invariant():
    var, gt, lab = _inputs()
    r = _full()
    pick = [0, 6, 8, 3]                                                     # (the smallest packing runs a pass per entry and image)
    small = var.attention_knockout(gt, lab, [EDGES[j] for j in pick], max_rows=2)
    _same(small, 0, r, 0, 'max_rows=2: the clean row')
    for i, j in enumerate(pick):
        _same(small, i + 1, r, j + 1, f'max_rows=2: {EDGES[j]}')
    perm = [9, 2, 5, 0, 7, 4, 10, 8, 1, 6, 3]
    other = var.attention_knockout(gt, lab, [EDGES[j] for j in perm], max_rows=17)          # an image per pass, its entries in one chunk
    _same(other, 0, r, 0, 'max_rows=17: the clean row')
    for i, j in enumerate(perm):
        _same(other, i + 1, r, j + 1, f'permuted: {EDGES[j]}')
    alone = var.attention_knockout(gt[1:2], lab[1:2], EDGES[:4])
    for k in FIELDS:
        assert torch.equal(bits(getattr(alone, k)[0]), bits(getattr(r, k)[1, :5])), f'image 1 alone: {k}'
    one = var.attention_knockout(gt, lab, [(8, 3)], layers=(5,))
    _same(one, 1, r, 8, '(8, 3) with layers=(5,) against (8, 3, 5)')


def test_no_logits_tensor():
    """d16, 4 images x (clean + 7 entries) = 32 rows in one pass: after a warm-up call the peak allocation rises by the call's own buffers (the
    gathered clean rows of one scale, the per-pass and the returned values, the gathered inputs) and less than a quarter of one (rows, L, V)
    tensor beside them"""
    var = d16()[1]
    gt = tokens(var, 4, 24)
    lab = torch.arange(4, device='cuda')
    var.attention_knockout(gt, lab, EDGES[:7], max_rows=32)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = var.attention_knockout(gt, lab, EDGES[:7], max_rows=32)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    R, M = 32, 32 * var.patch_nums[-1] ** 2
    full = R * var.L * var.V * 4
    own = M * var.V * 4 + (R + 4 * 8) * var.L * (4 * 3 + 8 + 4) + R * var.L * (var.Cvae * 4 + 8) + 4 * var.L * (var.Cvae * 4 * 4 + 8 * 2)
    assert r.nll.shape == (4, 8, var.L)
    print(f'peak rise {rise / 1e6:.1f} MB; own buffers {own / 1e6:.1f} MB; one (rows, L, V) tensor {full / 1e6:.1f} MB')
    assert rise < own + full // 4, f'peak allocation rose by {rise / 1e6:.1f} MB'


def test_refused_in_the_16_bit_modes():
    var, gt, lab = _inputs()
    for prec in ('f16', 'bf16'):
        var.set_hip_precision(prec)
        try:
            with pytest.raises(ValueError, match='attention_knockout runs in f32'):
                var.attention_knockout(gt, lab, EDGES[:2])
        finally:
            var.set_hip_precision('f32')


def test_pytorch_route_agrees():
    """the same model in train mode (the PyTorch route on the device) against eval mode (the HIP route), f32: nll, entropy and kl at evalref.BAR,
    the bar between the project's two routes; pred on the tokens whose top-2 margin in the PyTorch route's float64 logits exceeds
    2 * evalref.GAP, which must be 90 % of every row's tokens (checked on the PyTorch route alone, first)."""
    from var_amd.models import args as A
    from var_amd.models.var import attention_knockout_torch
    var, gt, lab = _inputs()
    a = _full()
    cuts = A.knockout_masks(a.edges, var.num_heads)
    margin = torch.empty(2, len(EDGES) + 1, var.L, dtype=torch.float64, device='cuda')

    def tap(n, j, z):
        t2 = z.double().topk(2, dim=-1).values
        margin[n, j] = t2[..., 0] - t2[..., 1]
    var.train()
    try:
        assert not var._scoring_on_hip(var.lvl_1L)
        with torch.no_grad():
            b = dict(zip(FIELDS, attention_knockout_torch(var, gt, lab, cuts, _tap=tap)))
            pub = var.attention_knockout(gt[:1], lab[:1], EDGES[:1])                    # the public call takes the twin here
    finally:
        var.eval()
    assert torch.equal(pub.nll[0], b['nll'][0, :2].float()) and torch.equal(pub.pred[0], b['pred'][0, :2])
    clear = margin > 2 * evalref.GAP
    lowest = float(clear.double().mean(-1).min())
    print(f'tokens with a top-2 margin above {2 * evalref.GAP}: {float(clear.double().mean()):.4f} (the lowest row: {lowest:.4f})')
    assert lowest >= 0.9
    worst = {}
    for k in ('nll', 'entropy', 'kl'):
        d = (getattr(a, k).double() - b[k].double()).abs()
        worst[k] = float(d.max())
        print(f'{k}: max |HIP - PyTorch| per row {[f"{v:.1e}" for v in d.amax(dim=(0, 2)).tolist()]}')
    for k, v in worst.items():
        assert v <= evalref.BAR, f'{k}: {v:.3e}'
    assert torch.equal(a.pred[clear], b['pred'][clear])
