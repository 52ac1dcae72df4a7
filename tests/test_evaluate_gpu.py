"""VAR.evaluate on the MI355X: varhip_token_eval_f32 and varhip_eval_reduce_f32 against float64 / torch, the end-to-end call against the
reference's logits and the engine's own teacher-forced logits (d16), one piece of code with token_log_likelihood (bit for bit), bitwise packing
invariance, no full logits tensor in memory, agreement with the PyTorch route, and the cached workspaces left as every other call expects."""
import contextlib

import numpy as np
import pytest
import torch

from tests import evalref, util
from tests.test_likelihood_gpu import d16, kernel_bar_ok, tokens          # (one d16 model for both files)
from var_amd import abi, hip

pytestmark = pytest.mark.gpu

SENT_F, SENT_I = 12345.0, -777


def _rows(V, R, l, seed):
    """R * l rows of logits with the corner cases planted, and their tokens (R, l)"""
    g = torch.Generator(device='cuda').manual_seed(seed)
    z = torch.randn(R * l, V, device='cuda', generator=g) * 6
    z[::5, :7] += 40                                        # a few peaked rows
    gt = torch.randint(0, V, (R, l), device='cuda', generator=g)
    f = gt.view(-1)
    z[2, 5] = z[2, V - 1] = 60.0; f[2] = V - 1              # an exact tie at the maximum, gt the higher index: pred 5, rank 1
    z[3, 9] = z[3, 700] = 60.0; f[3] = 9                    # ... gt the lower one: pred 9, rank 0
    z[4, 100] = z[4, 500] = z[4, 900] = 0.125; f[4] = 500   # gt tied with a code on either side of it, below the maximum
    z[6, 0] = 0.0; z[6, 1] = -0.0; z[6, 2:] = -3.0; f[6] = 1    # +0 == -0
    z[7, 33] = z[7, V - 2] = float('nan'); f[7] = 40        # a NaN row: pred 33, nll NaN, NaN compares false
    f[8] = -1; f[9] = V                                     # tokens outside [0, V): NaN, rank -1, never dereferenced
    return z, gt


def _token_eval_vs_float64(V, layout):
    R, l, N, L, r0, tok0 = layout
    z, gt_rows = _rows(V, R, l, V)
    gt = torch.randint(0, V, (N, L), device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    gt[r0:r0 + R, tok0:tok0 + l] = gt_rows
    nll, smooth = torch.full((N, L), SENT_F, device='cuda'), torch.full((N, L), SENT_F, device='cuda')
    pred = torch.full((N, L), SENT_I, dtype=torch.int64, device='cuda')
    rank = torch.full((N, L), SENT_I, dtype=torch.int32, device='cuda')
    util.guarded_call('token_eval_f32', z, gt[r0:, tok0:], L, R, l, V, nll[r0:, tok0:], smooth[r0:, tok0:], pred[r0:, tok0:], rank[r0:, tok0:], L)
    torch.cuda.synchronize()
    sl = (slice(r0, r0 + R), slice(tok0, tok0 + l))
    g = gt_rows.view(-1)
    valid = ((g >= 0) & (g < V)).cpu().numpy()
    zc = z.cpu().numpy()
    n64, s64, p_ref, r_ref = evalref.token_defs(zc[valid], g.cpu().numpy()[valid])
    got_nll, got_smooth = nll[sl].reshape(-1).cpu(), smooth[sl].reshape(-1).cpu()
    got_pred, got_rank = pred[sl].reshape(-1).cpu().numpy(), rank[sl].reshape(-1).cpu().numpy()
    # integers: exactly the definitions; pred is torch.argmax on every row, the out-of-range ones included
    assert np.array_equal(got_pred, z.argmax(-1).cpu().numpy()) and np.array_equal(got_pred[valid], p_ref)
    assert np.array_equal(got_rank[valid], r_ref) and (got_rank[~valid] == -1).all()
    assert (got_pred[2], got_rank[2], got_pred[3], got_rank[3], got_pred[6], got_rank[6], got_pred[7]) == (5, 1, 9, 0, 0, 1, 33)
    assert got_rank[4] == int((z[4] > 0.125).sum()) + 1
    # floats: NaN where defined, the rest within the bars.  On the row holding a NaN (gt itself is finite there) nll is by contract whatever
    # varhip_token_loglik_f32 gives (its register path drops a NaN element from the exponential sum, its scalar path propagates it): pinned
    # below against that kernel on every row, this one included
    nan_want = ~valid
    nan_want[7] = True
    assert np.array_equal(np.isnan(got_nll.numpy())[valid], np.isnan(got_nll.numpy())[valid] & (np.arange(R * l) == 7)[valid])
    assert np.isnan(got_nll.numpy())[~valid].all() and np.array_equal(np.isnan(got_smooth.numpy()), nan_want)
    lp = torch.full((R, 1, l), SENT_F, device='cuda')
    util.guarded_call('token_loglik_f32', z, gt_rows, l, R, 1, l, V, 0, 1.0, 0.0, lp, l, l)
    torch.cuda.synchronize()
    a, b = got_nll, -lp.view(-1).cpu()
    assert bool(((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all()), 'nll is not -token_loglik bit for bit'
    fin = torch.from_numpy(~nan_want)
    fin_v = torch.from_numpy(~nan_want[valid])
    zf = z.cpu()[fin]
    ok, err = kernel_bar_ok(-got_nll[fin], -torch.from_numpy(n64)[fin_v], zf)
    assert ok, f'V={V}: max |nll - nll64| {err:.3e} beyond the bar'
    serr = (got_smooth[fin].double() - torch.from_numpy(s64)[fin_v]).abs() - 1e-6 * (zf.abs().amax(-1).double() + 1)
    assert float(serr.max()) <= 0, f'V={V}: smooth beyond 1e-6 (max|z| + 1) by {float(serr.max()):.3e}'
    for out, sent in ((nll, SENT_F), (smooth, SENT_F), (pred, SENT_I), (rank, SENT_I)):
        untouched = torch.ones(N, L, dtype=torch.bool, device='cuda')
        untouched[sl] = False
        assert bool((out[untouched] == sent).all()), 'the kernel wrote outside its slice'


@pytest.mark.parametrize('V', [4096, 1000, 4099, 5000])
def test_token_eval_vs_float64(V):
    """3 x 7 rows (register path, small register path, misaligned scalar path, above the register limit) into slices of larger (N, L) outputs"""
    _token_eval_vs_float64(V, (3, 7, 5, 20, 1, 9))


@pytest.mark.parametrize('V', [4096, 4099])
def test_token_eval_slices_end_their_allocations(V):
    """the same with r0 + R == N and tok0 + l == L: the last row's tokens are the last elements of gt and of every output"""
    _token_eval_vs_float64(V, (3, 7, 3, 16, 0, 9))


def test_token_eval_float64_sum_does_not_depend_on_the_path():
    """the order of the float64 row sum depends on V alone: a misaligned copy of the rows (scalar path) gives the same smooth bits"""
    V = 4096
    z, gt = _rows(V, 3, 7, 3)
    buf = torch.empty(21 * V + 1, device='cuda')
    z_off = buf[1:].view(21, V)                            # 4 bytes off the 16-byte alignment
    z_off.copy_(z)
    outs = []
    for src in (z, z_off):
        o = [torch.empty(3, 7, device='cuda'), torch.empty(3, 7, device='cuda'), torch.empty(3, 7, dtype=torch.int64, device='cuda'),
             torch.empty(3, 7, dtype=torch.int32, device='cuda')]
        util.guarded_call('token_eval_f32', src, gt, 7, 3, 7, V, *o, 7)
        outs.append(o)
    torch.cuda.synchronize()
    (nll_a, *rest_a), (nll_b, *rest_b) = outs
    for a, b in zip(rest_a, rest_b):                       # smooth (NaN rows included: compared as bits), pred, rank
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    # (max / exp-sum keep the lane-strided order of the scalar path, as in k_token_loglik: both within the kernel's bar of float64, so within two bars)
    fin = torch.isfinite(nll_a) & torch.isfinite(nll_b) & torch.isfinite(z).all(-1).view(3, 7)
    two_bars = 2e-6 * (nll_a.abs().double() + z.abs().amax(-1).view(3, 7).double() + 8)
    assert int(fin.sum()) == 18 and bool(((nll_a.double() - nll_b.double()).abs()[fin] <= two_bars[fin]).all())


def test_token_eval_rejects_bad_sizes():
    lg = torch.zeros(8, 256, device='cuda'); gt = torch.zeros(2, 8, dtype=torch.int64, device='cuda')
    o = [torch.zeros(2, 8, device='cuda'), torch.zeros(2, 8, device='cuda'), torch.zeros(2, 8, dtype=torch.int64, device='cuda'),
         torch.zeros(2, 8, dtype=torch.int32, device='cuda')]
    f = hip.lib().fn['token_eval_f32']
    st = hip.current_stream()
    good = [lg.data_ptr(), gt.data_ptr(), 8, 2, 4, 256, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), 8]
    assert f(*good, st) == 0
    torch.cuda.synchronize()
    for pos, val in [(3, 0), (4, 0), (5, 0), (5, 1 << 24), (2, 3), (10, 3), (0, None), (1, None), (6, None), (7, None), (8, None), (9, None)]:
        a = list(good); a[pos] = val
        assert f(*a, st) == abi.EINVAL, (pos, val)


@pytest.mark.parametrize('pns,V', [((1, 2, 3), 4096), ((1, 2, 3, 4, 5), 4096), ((1, 2, 3), 10000)])
def test_eval_reduce(pns, V):
    """N = 3; V = 10000 takes the global-atomics histogram; the per-token arrays are slices of wider ones (ld > L)"""
    N, S, L = 3, len(pns), sum(p * p for p in pns)
    ld = L + 3
    g = torch.Generator(device='cuda').manual_seed(V + S)
    nll = (torch.rand(N, ld, device='cuda', generator=g) * 9 + 0.01)
    smooth = torch.randn(N, ld, device='cuda', generator=g) * 4 + 6
    pred = torch.randint(0, V, (N, ld), device='cuda', generator=g)
    pred[:, :3] = V - 1; pred[0, 3] = 0
    rank = torch.randint(-1, 3, (N, ld), device='cuda', generator=g).to(torch.int32)
    begins = torch.tensor(np.concatenate([[0], np.cumsum([p * p for p in pns])]), dtype=torch.int32)
    runs = []
    for _ in range(2):
        nll_S, smooth_S = torch.full((S,), -1.0, dtype=torch.float64, device='cuda'), torch.full((S,), -1.0, dtype=torch.float64, device='cuda')
        correct_S = torch.full((S,), -1, dtype=torch.int64, device='cuda')
        hist = torch.zeros(V, dtype=torch.int64, device='cuda')
        util.guarded_call('eval_reduce_f32', nll, smooth, pred, rank, ld, N, begins, S, V, nll_S, smooth_S, correct_S, hist)
        torch.cuda.synchronize()
        runs.append((nll_S, smooth_S, correct_S, hist))
    nll_S, smooth_S, correct_S, hist = runs[0]
    be = list(zip(begins[:-1].tolist(), begins[1:].tolist()))
    assert correct_S.tolist() == [int((rank[:, b:e] == 0).sum()) for b, e in be]
    assert torch.equal(hist, torch.bincount(pred[:, :L].reshape(-1), minlength=V))
    for got, src in ((nll_S, nll), (smooth_S, smooth)):
        want = np.array([src[:, b:e].cpu().numpy().astype(np.float64).sum() for b, e in be])
        rel = np.abs(got.cpu().numpy() - want) / np.abs(want)
        assert rel.max() <= 1e-12, f'float64 sums: relative error {rel.max():.3e}'
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)), 'two runs differ'


def test_eval_reduce_rejects_bad_sizes():
    N, L, V = 2, 14, 64
    a = [torch.zeros(N, L, device='cuda'), torch.zeros(N, L, device='cuda'), torch.zeros(N, L, dtype=torch.int64, device='cuda'),
         torch.zeros(N, L, dtype=torch.int32, device='cuda')]
    o = [torch.zeros(3, dtype=torch.float64, device='cuda'), torch.zeros(3, dtype=torch.float64, device='cuda'),
         torch.zeros(3, dtype=torch.int64, device='cuda'), torch.zeros(V, dtype=torch.int64, device='cuda')]
    begins, unsorted, nonzero = (torch.tensor(b, dtype=torch.int32) for b in ([0, 1, 5, 14], [0, 5, 5, 14], [1, 2, 5, 14]))
    f = hip.lib().fn['eval_reduce_f32']
    st = hip.current_stream()
    good = [t.data_ptr() for t in a] + [L, N, begins.data_ptr(), 3, V] + [t.data_ptr() for t in o]
    assert f(*good, st) == 0
    torch.cuda.synchronize()
    for pos, val in [(4, L - 1), (5, 0), (7, 0), (7, 33), (8, 0), (6, unsorted.data_ptr()), (6, nonzero.data_ptr()), (0, None), (3, None), (6, None),
                     (9, None), (12, None)]:
        b = list(good); b[pos] = val
        assert f(*b, st) == abi.EINVAL, (pos, val)


@contextlib.contextmanager
def precision(var, prec):
    var.set_hip_precision(prec)
    try:
        yield
    finally:
        var.set_hip_precision('f32')


INT_FIELDS = ('correct_S', 'tokens_S', 'pred_hist_V', 'pred_BL', 'rank_BL')


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


@pytest.mark.parametrize('prec', ['f32', 'f16', 'bf16'])
def test_nll_is_token_log_likelihood_bit_for_bit(prec):
    vae, var = d16()
    gt = tokens(var, 2, 21)
    lab = torch.tensor([207, 1000], device='cuda')
    with precision(var, prec):
        r = var.evaluate(gt, lab)
        lp = var.token_log_likelihood(gt, lab.view(2, 1))[:, 0]
    assert torch.equal(bits(r.nll_BL), bits(-lp))


@pytest.mark.parametrize('prec', ['f32', 'bf16'])
def test_d16_vs_engine_logits(prec):
    """L = 680: against the engine's own teacher-forced logits var(label, x) reduced in float64 and torch, same precision"""
    vae, var = d16()
    N, L, V = 2, var.L, var.V
    gt = tokens(var, N, 22)
    lab = torch.tensor([3, 999], device='cuda')
    with precision(var, prec), torch.no_grad():
        r = var.evaluate(gt, lab, label_smooth=0.1)
        # (inside no_grad, as evaluate computes it: with autograd on, idxBl_to_var_input takes its PyTorch branch, whose fp32 roundings differ)
        z = var(lab, vae.quantize.idxBl_to_var_input([gt[:, b:e] for b, e in var.begin_ends]))
    assert z.shape == (N, L, V) and z.dtype == torch.float32
    g = gt.unsqueeze(-1)
    nll64 = -z.double().log_softmax(-1).gather(-1, g).squeeze(-1)
    ok, err = kernel_bar_ok(-r.nll_BL, -nll64, z)
    assert ok, f'{prec}: max |nll - nll64| {err:.3e}'
    # both sides reduce the same logits bits: the integers agree on every row
    zg = z.gather(-1, g)
    rank = ((z > zg) | ((z == zg) & (torch.arange(V, device='cuda') < g))).sum(-1)
    same = (r.pred_BL == z.argmax(-1)) & (r.rank_BL == rank)
    assert int(same.sum()) == N * L, f'{prec}: pred / rank differ on {N * L - int(same.sum())} rows'
    # eval_ep's formulas (trainer.py:72-75) on that tensor, in float64; each mean within the mean of the per-token bars
    F = torch.nn.functional
    last = var.patch_nums[-1] ** 2
    bar = 1e-6 * (nll64.abs() + z.abs().amax(-1).double() + 8)
    assert abs(r.L_mean - float(F.cross_entropy(z.double().view(-1, V), gt.view(-1)))) <= float(bar.mean())
    assert abs(r.L_tail - float(F.cross_entropy(z.double()[:, -last:].reshape(-1, V), gt[:, -last:].reshape(-1)))) <= float(bar[:, -last:].mean())
    assert abs(r.acc_mean - float((z.argmax(-1) == gt).sum()) * 100 / L / N) < 1e-9
    assert abs(r.acc_tail - float((z[:, -last:].argmax(-1) == gt[:, -last:]).sum()) * 100 / last / N) < 1e-9
    want = float(F.cross_entropy(z.double().view(-1, V), gt.view(-1), label_smoothing=0.1))
    assert abs(r.loss - want) <= float(bar.mean()) + 0.1 * 1e-6 * (float(z.abs().max()) + 1)
    assert torch.equal(r.pred_hist_V, torch.bincount(z.argmax(-1).view(-1), minlength=V))


def test_reference_fixture_on_the_hip_route(golden_dir):
    vae, var = evalref.fixture_model(golden_dir, 'cuda')
    assert var._scoring_on_hip(var.lvl_1L)
    evalref.check_against_reference_fixture(var, golden_dir, 'cuda')


@pytest.mark.parametrize('prec', ['f32', 'bf16'])
def test_packing_is_bitwise_invariant(prec):
    vae, var = d16()
    gt = tokens(var, 3, 23)
    lab = torch.tensor([4, 1000, 31], device='cuda')
    with precision(var, prec):
        base = var.evaluate(gt, lab, label_smooth=0.1, max_rows=64)
        for mr in (1, 2):
            r = var.evaluate(gt, lab, label_smooth=0.1, max_rows=mr)
            for name in INT_FIELDS + ('nll_BL', 'nll_S', 'smooth_S'):
                assert torch.equal(bits(getattr(r, name)), bits(getattr(base, name))), f'{prec} max_rows={mr}: {name}'
        parts = [var.evaluate(gt[i:i + 1], lab[i:i + 1], label_smooth=0.1) for i in range(3)]
    s = parts[0] + parts[1] + parts[2]
    assert s.images == 3
    for name in INT_FIELDS + ('nll_BL',):
        assert torch.equal(bits(getattr(s, name)), bits(getattr(base, name))), f'{prec} per-image calls: {name}'
    for name in ('nll_S', 'smooth_S'):                       # (the order of a float64 sum is defined per call)
        x, y = getattr(s, name), getattr(base, name)
        assert float(((x - y).abs() / y.abs()).max()) <= 1e-12, f'{prec} per-image calls: {name}'


def test_no_full_logits_tensor():
    """d16, 8 images in one pass: after a warm-up call, the second call's peak allocation increase stays below a quarter of 8 * L * V * 4 bytes"""
    vae, var = d16()
    gt = tokens(var, 8, 24)
    lab = torch.arange(8, device='cuda')
    var.evaluate(gt, lab, max_rows=8)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = var.evaluate(gt, lab, max_rows=8)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    full = 8 * var.L * var.V * 4
    assert r.nll_BL.shape == (8, var.L) and bool(torch.isfinite(r.nll_BL).all())
    assert rise < full / 4, f'peak allocation rose by {rise / 1e6:.1f} MB (a full logits tensor is {full / 1e6:.0f} MB)'


def test_pytorch_route_agrees(golden_dir):
    """the fixture's model in train mode (the PyTorch route on the device, drop path off) against eval mode (the HIP route).  Both are within
    evalref.BAR of the reference's logits, so a gap between two logits moves by at most 2 * GAP between them: pred is equal on every row (the
    fixture's smallest top-2 gap is 1.45e-2), rank differs by at most the number of codes within 2 * GAP of z_gt in the reference's row.
    The window is deliberately twice that of the check against the reference itself (GAP): there one side is exact, here neither is."""
    from var_amd.models.helpers import DropPath
    vae, var = evalref.fixture_model(golden_dir, 'cuda')
    meta, gt, ref = evalref.fixture(golden_dir)
    for m in var.modules():
        if isinstance(m, DropPath):
            m.drop_prob = 0.0
    a = var.evaluate(gt.cuda(), meta['labels'], label_smooth=0.1)
    var.train()
    try:
        assert not var._scoring_on_hip(var.lvl_1L)
        b = var.evaluate(gt.cuda(), meta['labels'], label_smooth=0.1)
    finally:
        var.eval()
    assert float((a.nll_BL - b.nll_BL).abs().max()) <= evalref.BAR
    assert abs(a.L_mean - b.L_mean) <= evalref.BAR and abs(a.L_tail - b.L_tail) <= evalref.BAR and abs(a.loss - b.loss) <= evalref.BAR
    assert torch.equal(a.pred_BL, b.pred_BL) and torch.equal(a.pred_hist_V, b.pred_hist_V) and torch.equal(a.tokens_S, b.tokens_S)
    assert torch.equal(a.correct_S, b.correct_S)
    zg = np.take_along_axis(ref.numpy(), gt.numpy()[..., None], -1)
    near = (np.abs(ref.numpy() - zg) <= 2 * evalref.GAP).sum(-1) - 1
    drank = (a.rank_BL.long() - b.rank_BL.long()).abs().cpu().numpy()
    assert (drank <= near).all()


def test_leaves_the_cached_workspaces_as_other_calls_expect():
    """evaluate shares _tf_workspace with forward() and the scoring calls: each of them gives the same bits before and after it, and
    evaluate the same bits before and after them"""
    vae, var = d16()
    gt = tokens(var, 2, 25)
    lab = torch.tensor([5, 6], device='cuda')
    with torch.no_grad():
        x = vae.quantize.idxBl_to_var_input([gt[:, b:e] for b, e in var.begin_ends])
        lp0, z0 = var.token_log_likelihood(gt, [5, 6, 7], cfg=1.5), var(lab, x)
        r0 = var.evaluate(gt, lab)
        lp1, z1 = var.token_log_likelihood(gt, [5, 6, 7], cfg=1.5), var(lab, x)
        r1 = var.evaluate(gt, lab, max_rows=1)
    assert torch.equal(bits(lp0), bits(lp1)) and torch.equal(bits(z0), bits(z1))
    for name in INT_FIELDS + ('nll_BL', 'nll_S', 'smooth_S'):
        assert torch.equal(bits(getattr(r0, name)), bits(getattr(r1, name))), name
