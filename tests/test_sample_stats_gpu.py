"""varhip_sample_stats_f32 on the MI355X: bit-equal to its host twin, bit-equal to varhip_token_loglik_f32 on the same rows,
within the derived bounds of float64 (tests/samplestatsref.py), and the identities that tie it to the sampler whose operands it reads.
Shapes: B in {1, 3}, l in {1, 4} (one wave, a partly filled workgroup, more than one workgroup), V in {256, 4096, 8192} (the three row paths)."""
import numpy as np
import pytest
import torch

from tests import samplestatsref as R
from tests import util
from tests.test_sample_stats_cpu import host_stats
from var_amd import abi, hip

pytestmark = pytest.mark.gpu

CASES = [(1, 1), (1, 4), (3, 1), (3, 4)]
TS = [0.0, 1.5, 0.3333333333333333]


def gpu_stats(logits, masked, idx, B, l, V, t, t_rows=None, ld_out=None):
    """numpy / torch operands -> dict of (B, ld_out) numpy arrays, the call made through guard arenas"""
    ld = l if ld_out is None else ld_out
    dev = lambda a: a.cuda() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = {k: torch.full((B, ld), -77, dtype=torch.int32 if k == 'kept' else torch.float32, device='cuda') for k, _ in R.FIELDS}
    tr = None if t_rows is None else torch.tensor(list(t_rows), dtype=torch.float64, device='cuda')
    util.guarded_call('sample_stats_f32', dev(logits), dev(masked), dev(idx), B, l, V, float(t), tr,
                      out['lp_cond'], out['lp_guided'], out['lp_drawn'], out['kept'], out['entropy'], ld)
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits_equal(a, b):
    """the same bits, or a NaN on both sides (a NaN's sign and payload carry nothing)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != np.float32:
        return np.array_equal(a, b)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize('V', [256, 4096, 8192])
@pytest.mark.parametrize('B, l', CASES)
def test_kernel_equals_host_twin_token_loglik_and_float64(B, l, V):
    t, ld = 1.25, l + 3
    logits, masked, idx = R.make_case(B, l, V, t, 37, seed=B * 100 + l * 10 + V)
    if B == 3:
        idx[0] = -1                                                     # a refused image's row: never dereferenced
        logits[l, 3] = np.nan                                           # a NaN in a conditional row, the token elsewhere
    got = gpu_stats(logits, masked, idx, B, l, V, t, ld_out=ld)
    host = host_stats(logits, masked, idx, B, l, V, t, ld_out=ld)
    for k, _ in R.FIELDS:
        assert bits_equal(got[k], host[k]), f'{k}: the kernel differs from its host twin (the untouched columns past l included)'
    # one piece of device code with the teacher-forced scorer: the same rows through varhip_token_loglik_f32
    lg, gt = torch.from_numpy(logits).cuda(), torch.from_numpy(idx).cuda().view(B, l)
    for key, u, ca, cb in (('lp_cond', 0, 1.0, 0.0), ('lp_guided', 1, float(np.float32(1.0 + t)), float(np.float32(t)))):
        lp = torch.full((B, 1, l), -77.0, device='cuda')
        util.guarded_call('token_loglik_f32', lg, gt, l, B, 1, l, V, u, ca, cb, lp, l, l)
        assert bits_equal(got[key][:, :l], lp.view(B, l).cpu().numpy()), f'{key} is not varhip_token_loglik_f32 bit for bit'
    clean = np.ones((B, l), bool)
    if B == 3:
        clean[1, 0] = False                                             # the NaN row: pinned by the two bitwise checks above
        assert np.isnan(got['lp_cond'][0, 0]) and np.isnan(got['lp_drawn'][0, 0]) and got['kept'][0, 0] == 37 and np.isnan(got['entropy'][1, 0])
    ref = R.reference(logits, masked, idx, B, l, t)
    R.check_against_reference({k: v[:, :l][clean] for k, v in got.items()}, {k: v[clean] for k, v in ref.items()}, V)


@pytest.mark.parametrize('V', [256, 4096, 8192])
def test_device_array_form_equals_the_scalar_form_per_image(V):
    B, l = 3, 4
    logits, _, _ = R.make_case(B, l, V, 0.0, V, seed=V + 1)
    masked = R.filtered(R.guided_rows(logits, B, l, TS), 40)
    idx = np.array([np.flatnonzero(r != -np.inf)[3] for r in masked], np.int64)
    got = gpu_stats(logits, masked, idx, B, l, V, 99.0, t_rows=TS)       # (the scalar is not read)
    R.check_against_reference(got, R.reference(logits, masked, idx, B, l, TS), V)
    lg = logits.reshape(2, B, l, V)
    for b in range(B):
        one = gpu_stats(lg[:, b].reshape(2 * l, V), masked[b * l:(b + 1) * l], idx[b * l:(b + 1) * l], 1, l, V, TS[b])
        for k, _ in R.FIELDS:
            assert bits_equal(one[k][0], got[k][b]), f'image {b}, {k}: the array form differs from the scalar form on its rows alone'


@pytest.mark.parametrize('V', [256, 4096, 8192])
@pytest.mark.parametrize('B, l', [(1, 1), (3, 4)])
def test_behind_the_sampler(B, l, V):
    """the sampler, then the stats kernel on its masked_out / idx_out.  top_k = 1: one code kept, drawn with probability 1.  No filter: every
    code kept, the drawn distribution is the guided one (the same code on the same floats).  Any filter only removes mass, so
    lp_drawn >= lp_guided up to the two values' own error bounds."""
    t = 1.5
    g = torch.Generator(device='cuda').manual_seed(V + B)
    logits = torch.randn(2 * B * l, V, device='cuda', generator=g) * 3
    noise = torch.empty(B * l, V, device='cuda').exponential_(1, generator=g)
    for top_k, top_p in ((1, 0.0), (0, 0.0), (50, 0.0), (0, 0.9), (200, 0.96)):
        idx = torch.full((B * l,), -5, dtype=torch.int64, device='cuda')
        masked = torch.full((B * l, V), 7.0, device='cuda')
        util.guarded_call('cfg_sample_f32', logits, noise, idx, masked, B, l, V, t, top_k, top_p)
        got = gpu_stats(logits, masked, idx, B, l, V, t)
        what = f'top_k={top_k} top_p={top_p}'
        assert np.isfinite(got['lp_drawn']).all() and (got['lp_drawn'] <= 0).all(), what
        if top_k == 1:
            assert (got['kept'] == 1).all() and (got['lp_drawn'] == 0.0).all(), what
        if top_k == 0 and top_p == 0.0:
            assert (got['kept'] == V).all() and bits_equal(got['lp_drawn'], got['lp_guided']), what
        if top_k > 0:
            assert (got['kept'] >= 1).all() and (got['kept'] <= top_k).all(), what
        slack = R.lp_bound(got['lp_drawn'].astype(np.float64), V) + R.lp_bound(got['lp_guided'].astype(np.float64), V)
        assert (got['lp_drawn'].astype(np.float64) >= got['lp_guided'].astype(np.float64) - slack).all(), what
        R.check_against_reference(got, R.reference(logits.cpu().numpy(), masked.cpu().numpy(), idx.cpu().numpy(), B, l, t), V, what + ': ')


def test_per_image_sampler_then_stats_with_a_refused_image():
    """varhip_cfg_sample_rows_f32 with its device tables, image 1 refused (top_k beyond the launch's cap): idx -1 there, masked left alone"""
    B, l, V = 3, 4, 4096
    g = torch.Generator(device='cuda').manual_seed(11)
    logits = torch.randn(2 * B * l, V, device='cuda', generator=g) * 3
    noise = torch.empty(B * l, V, device='cuda').exponential_(1, generator=g)
    tt = torch.tensor(TS, dtype=torch.float64, device='cuda')
    tk = torch.tensor([8, 900, 1], dtype=torch.int32, device='cuda')
    tp = torch.tensor([0.0, 0.0, 0.0], dtype=torch.float64, device='cuda')
    idx = torch.full((B * l,), -5, dtype=torch.int64, device='cuda')
    masked = torch.zeros(B * l, V, device='cuda')
    util.guarded_call('cfg_sample_rows_f32', logits, noise, idx, masked, B, l, V, tt, tk, tp, 8)
    assert (idx.view(B, l)[1] == -1).all()
    got = gpu_stats(logits, masked, idx, B, l, V, 0.0, t_rows=TS)
    for k in ('lp_cond', 'lp_guided', 'lp_drawn'):
        assert np.isnan(got[k][1]).all() and np.isfinite(got[k][[0, 2]]).all(), k
    assert (got['kept'][0] == 8).all() and (got['kept'][1] == V).all() and (got['kept'][2] == 1).all() and np.isfinite(got['entropy']).all()
    R.check_against_reference(got, R.reference(logits.cpu().numpy(), masked.cpu().numpy(), idx.cpu().numpy(), B, l, TS), V)


def test_kernel_rejects_bad_arguments():
    B, l, V = 1, 2, 256
    lg = torch.zeros(2 * B * l * V + 4, device='cuda'); mk = torch.zeros(B * l * V + 4, device='cuda')
    ix = torch.zeros(B * l, dtype=torch.int64, device='cuda')
    o = [torch.zeros(B, l, dtype=torch.int32 if i == 3 else torch.float32, device='cuda') for i in range(5)]
    f, st = hip.lib().fn['sample_stats_f32'], hip.current_stream()
    good = [lg.data_ptr(), mk.data_ptr(), ix.data_ptr(), B, l, V, 1.0, None] + [x.data_ptr() for x in o] + [l]
    assert f(*good, st) == 0
    torch.cuda.synchronize()
    bad = [(0, None), (1, None), (2, None), (8, None), (9, None), (10, None), (11, None), (12, None), (3, 0), (4, 0), (5, 0), (5, 255), (5, 8448),
           (13, l - 1), (0, lg.data_ptr() + 4), (1, mk.data_ptr() + 4)]
    for pos, val in bad:
        a = list(good); a[pos] = val
        assert f(*a, st) == abi.EINVAL, (pos, val)
