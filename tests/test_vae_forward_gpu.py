"""VQVAE.forward / forward_stats on the HIP path: the new kernels alone (through the guard bands of tests/util.py), bit-for-bit
consistency with the encode / decode entry points that exist, the reference's fixtures (tests/golden/vaefwd_*.npz), history independence and
routing."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import util
from tests.test_vae_forward_cpu import CASES, build_vae, load

pytestmark = pytest.mark.gpu

# Relative deviation of mse_S / vq_loss from the reference's fixture values: 8 x the worst value measured over the fixtures a-d on an MI355X
# (mse_S 4.8e-7 at d_b3, vq_loss 3.3e-7 at d_b3 — a few fp32 ulps: the reference sums the squares in fp32 in torch's order, the
# kernel sums in float64 and rounds once, and the encoder's f differs from the reference's in its last bits).  The call is deterministic: the
# margin covers other weights and inputs.  Each test prints the value it measured (MEASURED ...) before it asserts.
MSE_REL_BOUND, LOSS_REL_BOUND = 8 * 4.8e-7, 8 * 3.3e-7
# rec: the atol of the fp32 image checks against the reference in tests/test_e2e_gpu.py (`image vs reference`, atol=1e-3);
# f_hat_st: that of its `f_hat (last) vs reference` check (atol=2e-5, rtol=1e-5)
REC_ATOL, FHAT_ATOL, FHAT_RTOL = 1e-3, 2e-5, 1e-5


def _stats(f_hat, f, idx, V, sum_out=True):
    dev = f.device
    hits = torch.zeros(V, dtype=torch.int64, device=dev)
    scratch = torch.zeros(1024, dtype=torch.float64, device=dev)
    s = torch.zeros(1, dtype=torch.float64, device=dev)
    mse = torch.zeros(1, dtype=torch.float32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    util.guarded_call('vq_scale_stats_f32', f_hat, f, f.numel(), idx, idx.numel(), V, hits, scratch, s if sum_out else None, mse, bad)
    return hits, s, mse, bad


def _idx(kind, n, V, g):
    if kind == 'uniform':
        return torch.randint(0, V, (n,), generator=g)
    if kind == 'one':
        return torch.full((n,), V - 1, dtype=torch.int64)
    return torch.cat([torch.randperm(V, generator=g) for _ in range((n + V - 1) // V)])[:n]


@pytest.mark.parametrize('kind', ['uniform', 'one', 'perm'])
@pytest.mark.parametrize('B,P,C,V', [(2, 4, 8, 4096), (3, 16, 32, 4096), (64, 16, 32, 4096), (2, 13, 32, 4096), (3, 5, 32, 10000)])
def test_scale_stats_kernel(B, P, C, V, kind):
    g = torch.Generator().manual_seed(B * 1000 + P)
    f_hat, f = torch.randn(B, P, P, C, generator=g), torch.randn(B, P, P, C, generator=g)
    idx = _idx(kind, B * P * P, V, g)
    hits, s, mse, bad = _stats(f_hat.cuda(), f.cuda(), idx.cuda(), V)
    assert torch.equal(hits.cpu(), torch.bincount(idx, minlength=V)) and int(bad) == 0
    n = f.numel()
    want = ((f_hat.numpy().astype(np.float64) - f.numpy().astype(np.float64)) ** 2).sum()
    rel = abs(float(s) - want) / want
    print(f'sum rel {rel:.2e}')
    assert rel <= 1e-9                                              # any-order fp64 sum of n <= 2^22 non-negative terms: <= n 2^-53 ~ 5e-10
    assert mse.cpu().numpy()[0].tobytes() == np.float32(float(s) / n).tobytes()
    hits2, s2, mse2, _ = _stats(f_hat.cuda(), f.cuda(), idx.cuda(), V, sum_out=False)
    assert torch.equal(hits2, hits) and mse2.cpu().numpy().tobytes() == mse.cpu().numpy().tobytes() and float(s2) == 0.0
    _, s3, _, _ = _stats(f_hat.cuda(), f.cuda(), idx.cuda(), V)
    assert s3.cpu().numpy().tobytes() == s.cpu().numpy().tobytes()  # run to run: equal bits


@pytest.mark.parametrize('V', [4096, 10000])
def test_scale_stats_reports_an_out_of_range_index(V):
    g = torch.Generator().manual_seed(1)
    f_hat, f = torch.randn(2, 4, 4, 8, generator=g), torch.randn(2, 4, 4, 8, generator=g)
    idx = torch.randint(0, V, (3000,), generator=g)
    idx[[0, 17, 1023, 1024, 2999]] = torch.tensor([-1, V, 1 << 40, -(1 << 40), V + 7])
    hits, _, _, bad = _stats(f_hat.cuda(), f.cuda(), idx.cuda(), V)
    ok = (idx >= 0) & (idx < V)
    assert int(bad) == 5 and torch.equal(hits.cpu(), torch.bincount(idx[ok], minlength=V)) and int(hits.sum()) == 2995


@pytest.mark.parametrize('B,P,C', [(2, 4, 8), (3, 13, 32), (64, 16, 32)])
def test_straight_through_kernel(B, P, C):
    g = torch.Generator().manual_seed(P)
    f_hat, f = torch.randn(B, P, P, C, generator=g).cuda(), (3 * torch.randn(B, P, P, C, generator=g)).cuda()
    want = (f_hat - f) + f
    assert not torch.equal(want, f_hat)                             # two roundings: not the identity
    a, b = torch.zeros_like(f), torch.zeros(B, C, P, P, device='cuda')
    util.guarded_call('vq_straight_through_f32', f_hat, f, a, b, B, P * P, C)
    assert torch.equal(a, want) and torch.equal(b, want.permute(0, 3, 1, 2))
    a2 = torch.zeros_like(f)
    util.guarded_call('vq_straight_through_f32', f_hat, f, a2, None, B, P * P, C)
    b2 = torch.zeros_like(b)
    util.guarded_call('vq_straight_through_f32', f_hat, f, None, b2, B, P * P, C)
    assert torch.equal(a2, want) and torch.equal(b2, b)


def test_loss_combine_kernel():
    mse = torch.rand(10, generator=torch.Generator().manual_seed(2)).cuda()
    out = torch.zeros(1, device='cuda')
    util.guarded_call('vq_loss_combine_f32', mse, 10, 0.25, out)
    assert torch.equal(out[0], _loss_sequence(mse, 0.25))


def _loss_sequence(mse_S, beta):
    """quant.py:95,97 over mse_S with torch scalar ops on the device, fp32, one kernel per operation"""
    acc = torch.zeros((), dtype=torch.float32, device=mse_S.device)
    for m in mse_S:
        acc = acc + (m * beta + m)
    return acc * (1. / len(mse_S))


def _same(a, b):
    assert all(torch.equal(x, y) for x, y in zip(a.idx_Bl, b.idx_Bl))
    for k in ('f_hat', 'hits_SV', 'mse_S', 'vq_loss', 'rec'):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


@pytest.mark.parametrize('name', ['a_l2', 'b_znorm', 'd_b3'])
def test_consistent_with_the_existing_entry_points(name):
    z, meta = load(name)
    vae = build_vae(meta, 'cuda').eval()
    img = torch.from_numpy(z['img']).cuda()
    pns, S = tuple(meta['patch_nums']), len(meta['patch_nums'])
    with torch.inference_mode():
        assert vae._forward_on_hip(img)
        st = vae.forward_stats(img)
        idx, fhs, post = vae.img_to_idxBl(img), vae.img_to_fhat(img), vae.img_to_post(img)
        raw = vae.quantize.hip_engine().quantize_stats(vae._encoder_engine().encode(img), pns, vae.quantize.beta)
        rec = vae(img)[0]
        assert all(torch.equal(a, b) for a, b in zip(st.idx_Bl, idx)) and len(idx) == S
        assert torch.equal(raw['f_hat_raw'].permute(0, 3, 1, 2), fhs[-1])
        assert torch.equal(raw['f_hat_st'], st.f_hat) and torch.equal(st.f_hat, (fhs[-1] - post) + post)
        assert torch.equal(rec, st.rec) and float(rec.abs().max()) > 1.0
        assert torch.equal(rec.clamp(-1, 1), vae.fhat_to_img(st.f_hat))            # same kernels, only the epilogue differs
        assert torch.equal(st.hits_SV, torch.stack([torch.bincount(i.reshape(-1), minlength=meta['V']) for i in idx]))
        n = post.numel()
        for si in range(S):
            want = ((fhs[si].cpu().numpy().astype(np.float64) - post.cpu().numpy().astype(np.float64)) ** 2).sum()
            got = float(raw['sum_S'][si])
            assert abs(got - want) <= 1e-9 * want, si
            assert st.mse_S[si].cpu().numpy().tobytes() == np.float32(got / n).tobytes() == raw['mse_S'][si].cpu().numpy().tobytes()
        assert torch.equal(st.vq_loss, _loss_sequence(st.mse_S, vae.quantize.beta))
        assert int(raw['bad']) == 0
        q = vae.quantize(post, ret_usages=True)                                    # the quantizer's own forward: the same bits from an NCHW map
        assert torch.equal(q[0], st.f_hat) and torch.equal(q[2], st.vq_loss)


@pytest.mark.parametrize('name', CASES)
def test_against_the_reference_fixtures(name):
    z, meta = load(name)
    vae = build_vae(meta, 'cuda').eval()
    vae.quantize.ema_vocab_hit_SV.copy_(torch.from_numpy(z['ema']))
    img = torch.from_numpy(z['img']).cuda()
    with torch.inference_mode():
        st = vae.forward_stats(img)
        rec, usages, vq_loss = vae(img, ret_usages=True)
    for si, i in enumerate(st.idx_Bl):
        ok, m = util.diff_report(f'{name} tokens s{si} vs reference', i.cpu().numpy().astype(np.int32), z[f'idx_s{si}']); print(m); assert ok, m
    assert np.array_equal(st.hits_SV.cpu().numpy(), z['hits_SV'])
    assert usages == list(z['usages'])
    ok, m = util.diff_report(f'{name} rec vs reference', rec.cpu().numpy(), z['rec'], atol=REC_ATOL); print(m); assert ok, m
    ok, m = util.diff_report(f'{name} f_hat_st vs reference', st.f_hat.cpu().numpy(), z['f_hat_st'], atol=FHAT_ATOL, rtol=FHAT_RTOL); print(m); assert ok, m
    rel_m = float(np.abs(st.mse_S.cpu().numpy().astype(np.float64) / z['mse_S'].astype(np.float64) - 1).max())
    rel_l = abs(float(vq_loss) / float(z['vq_loss']) - 1)
    print(f'MEASURED {name}: mse_S rel {rel_m:.3e} vq_loss rel {rel_l:.3e}')
    assert rel_m <= MSE_REL_BOUND and rel_l <= LOSS_REL_BOUND


def _models(meta):
    from models import build_vae_var
    from var_amd.detinit import fill_module_
    with contextlib.redirect_stdout(io.StringIO()):
        vae, var = build_vae_var(device='cuda', patch_nums=tuple(meta['patch_nums']), depth=2, ch=meta['ch'])
    fill_module_(var, 2, 0, 'var.'); fill_module_(vae, 2, 0, 'vae.')
    return vae.eval(), var.eval()


def test_history_independence():
    z, meta = load('a_l2')
    img = torch.from_numpy(z['img']).cuda()
    lab = torch.tensor([3, 7], device='cuda')
    kw = dict(g_seed=0, cfg=1.5, top_k=900, top_p=0.96)
    with torch.inference_mode():
        vae, var = _models(meta)
        first = vae.forward_stats(img)                               # the first call on a fresh model
        _same(first, vae.forward_stats(img))                         # repeated
        vae, var = _models(meta)
        tok0, smp0 = vae.img_to_idxBl(img), var.autoregressive_infer_cfg(2, lab, **kw)
        _same(first, vae.forward_stats(img))                         # after img_to_idxBl and a sampling call
        tok1, smp1 = vae.img_to_idxBl(img), var.autoregressive_infer_cfg(2, lab, **kw)
        assert all(torch.equal(a, b) for a, b in zip(tok0, tok1)) and torch.equal(smp0, smp1)       # and they are what they were before it
        _same(first, vae.forward_stats(img))
        # a .data edit of the codebook + invalidate_engines(): the result is that of a fresh model with the edited codebook
        vae.quantize.embedding.weight.data.mul_(0.5)
        vae.invalidate_engines()
        edited = vae.forward_stats(img)
        assert not torch.equal(edited.vq_loss, first.vq_loss)
        fresh, _ = _models(meta)
        fresh.quantize.embedding.weight.data.mul_(0.5)
        _same(edited, fresh.forward_stats(img))


def test_routing_grad_enabled_and_half_inputs_take_pytorch():
    z, meta = load('a_l2')
    vae = build_vae(meta, 'cuda').eval()
    img = torch.from_numpy(z['img']).cuda()
    with torch.inference_mode():
        hipr = vae.forward_stats(img)
    with torch.enable_grad():
        assert not vae._forward_on_hip(img)
        pt = vae.forward_stats(img)
    assert all(torch.equal(a, b) for a, b in zip(hipr.idx_Bl, pt.idx_Bl)) and torch.equal(hipr.hits_SV, pt.hits_SV)
    ok, m = util.diff_report('rec: PyTorch branch vs HIP', pt.rec.detach().cpu().numpy(), hipr.rec.cpu().numpy(), atol=REC_ATOL); print(m); assert ok, m
    ok, m = util.diff_report('f_hat_st: PyTorch branch vs HIP', pt.f_hat.detach().cpu().numpy(), hipr.f_hat.cpu().numpy(), atol=FHAT_ATOL, rtol=FHAT_RTOL); print(m); assert ok, m
    rel_m = float((pt.mse_S.detach().double() / hipr.mse_S.double() - 1).abs().max())
    rel_l = abs(float(pt.vq_loss) / float(hipr.vq_loss) - 1)
    print(f'MEASURED routing fp32: mse_S rel {rel_m:.3e} vq_loss rel {rel_l:.3e}')
    assert rel_m <= MSE_REL_BOUND and rel_l <= LOSS_REL_BOUND
    # a half map: cast to fp32 by contract, on the PyTorch branch; the HIP route on the same rounded values agrees
    f16 = torch.from_numpy(z['f']).cuda().half()
    with torch.inference_mode():
        assert not vae.quantize._forward_on_hip(f16) and vae.quantize._forward_on_hip(f16.float())
        a = vae.quantize.forward_stats(f16)
        b = vae.quantize.forward_stats(f16.float())
    assert a.f_hat.dtype == torch.float32
    assert all(torch.equal(x, y) for x, y in zip(a.idx_Bl, b.idx_Bl)) and torch.equal(a.hits_SV, b.hits_SV)
    ok, m = util.diff_report('half: f_hat_st PyTorch vs HIP', a.f_hat.cpu().numpy(), b.f_hat.cpu().numpy(), atol=FHAT_ATOL, rtol=FHAT_RTOL); print(m); assert ok, m
    rel_m = float((a.mse_S.double() / b.mse_S.double() - 1).abs().max())
    rel_l = abs(float(a.vq_loss) / float(b.vq_loss) - 1)
    print(f'MEASURED routing half: mse_S rel {rel_m:.3e} vq_loss rel {rel_l:.3e}')
    assert rel_m <= MSE_REL_BOUND and rel_l <= LOSS_REL_BOUND
