"""VQVAE.forward / VectorQuantizer2.forward and their forward_stats without a GPU: the PyTorch branch against the reference's
own outputs (tests/golden/vaefwd_*.npz, tools/gen_golden_vae_forward.py), its autograd wiring, the usages without a process group, the EMA
schedule under the package's dist flag, and the ABI of the new entry points."""
import glob
import json
import os
import tempfile

import numpy as np
import pytest
import torch

from tests import util
from tests.util import ROOT

CASES = ['a_l2', 'b_znorm', 'c_qsr0', 'c_qsr1', 'd_b3']


def load(name):
    z = np.load(os.path.join(util.GOLD, f'vaefwd_{name}.npz'))
    return z, json.loads(str(z['meta']))


def build_vae(meta, device='cpu', test_mode=True):
    from models.vqvae import VQVAE
    from var_amd.detinit import fill_module_
    vae = VQVAE(vocab_size=meta['V'], z_channels=meta['Cvae'], ch=meta['ch'], test_mode=test_mode, share_quant_resi=meta['share_quant_resi'],
                v_patch_nums=tuple(meta['patch_nums']), using_znorm=meta['using_znorm']).to(device)
    fill_module_(vae, 2, 0, 'vae.')
    return vae


def close(got, want):
    """the comparison of tests/test_host_cpu.py's encode-side checks against the reference (np.allclose, atol 1e-5, numpy's default rtol 1e-5)"""
    return np.allclose(np.asarray(got), np.asarray(want), atol=1e-5)


@pytest.mark.parametrize('name', CASES)
def test_torch_branch_against_the_reference(name):
    z, meta = load(name)
    vae = build_vae(meta).eval()
    vae.quantize.ema_vocab_hit_SV.copy_(torch.from_numpy(z['ema']))
    img = torch.from_numpy(z['img'])
    with torch.no_grad():
        st = vae.forward_stats(img)
        rec, usages, vq_loss = vae(img, ret_usages=True)
        f_hat, us2, vq2 = vae.quantize(torch.from_numpy(z['f']), ret_usages=True)
    assert len(st.idx_Bl) == len(meta['patch_nums'])
    for si, idx in enumerate(st.idx_Bl):
        assert idx.dtype == torch.int64 and np.array_equal(idx.numpy(), z[f'idx_s{si}']), si
    assert st.hits_SV.dtype == torch.int64 and np.array_equal(st.hits_SV.numpy(), z['hits_SV'])
    assert usages == list(z['usages']) and us2 == usages and any(u > 0 for u in usages)
    # the same torch on the same CPU: bit-equal to the reference
    assert np.array_equal(st.mse_S.numpy(), z['mse_S'])
    assert np.float32(vq_loss.item()) == z['vq_loss'] and float(st.vq_loss) == float(vq_loss) == float(vq2)
    assert np.array_equal(f_hat.numpy(), z['f_hat_st']) and np.array_equal(st.f_hat.numpy(), z['f_hat_st'])
    assert np.array_equal(rec.numpy(), z['rec']) and np.array_equal(st.rec.numpy(), z['rec'])
    assert close(rec.numpy(), z['rec']) and close(st.mse_S.numpy(), z['mse_S'])
    assert float(np.abs(z['rec']).max()) > 1.0                      # the fixture pins that forward does NOT clamp
    assert vae(img)[1] is None


def test_gradients_against_the_reference():
    z, meta = load('e_grad')
    vae = build_vae(meta, test_mode=False).train()
    vae.quantize.ema_vocab_hit_SV.copy_(torch.from_numpy(z['ema']))
    rec, usages, vq_loss = vae(torch.from_numpy(z['img']), ret_usages=True)
    assert np.array_equal(rec.detach().numpy(), z['rec']) and np.float32(vq_loss.item()) == z['vq_loss'] and usages == list(z['usages'])
    loss = vq_loss + rec.square().mean()
    loss.backward()
    assert np.float32(loss.item()) == z['loss']
    params = dict(vae.named_parameters())
    for n in meta['grad_names']:
        g = params[n].grad
        assert g is not None and float(g.abs().max()) > 0, n
        assert close(g.numpy(), z['grad.' + n]), (n, float(np.abs(g.numpy() - z['grad.' + n]).max()))
    assert vae.quantize.record_hit == 0                             # the package's dist is not initialised: no EMA update


def test_straight_through_and_the_two_loss_terms():
    z, meta = load('a_l2')
    vae = build_vae(meta, test_mode=False).train()
    q = vae.quantize
    f = torch.from_numpy(z['f']).clone().requires_grad_(True)
    f_hat, _, _ = q(f)
    cot = torch.randn(f.shape, generator=torch.Generator().manual_seed(5))
    (g,) = torch.autograd.grad(f_hat, f, cot)
    assert torch.equal(g, cot)                                      # d f_hat_st / d f is the identity
    phis = [p for phi in q.quant_resi.phis() for p in phi.parameters()]
    book = [q.embedding.weight] + phis

    def grads(beta, detach_f):
        q.beta = beta
        q.zero_grad()
        ff = torch.from_numpy(z['f']).clone().requires_grad_(not detach_f)
        loss = q(ff)[2]
        loss.backward()
        return (None if detach_f else ff.grad), [p.grad.clone() for p in book]
    gf, gb = grads(0.25, False)
    gf0, gb0 = grads(0.0, False)
    assert float(gf.abs().max()) > 0 and float(gf0.abs().max()) == 0.0          # f hears the commitment term only: beta = 0 silences it
    for a, b in zip(gb, gb0):
        assert torch.equal(a, b) and float(a.abs().max()) > 0                 # codebook / Phi hear the codebook term only: beta changes nothing
    _, gbd = grads(0.25, True)                                                 # f detached: the codebook side is unchanged
    for a, b in zip(gb, gbd):
        assert torch.equal(a, b)
    # the loss value is the fp32 sequence of DESIGN.md §20 over mse_S
    q.beta = 0.25
    with torch.no_grad():
        st = q.forward_stats(torch.from_numpy(z['f']))
    acc = np.float32(0.0)
    for m in st.mse_S.numpy():
        acc = np.float32(acc + np.float32(np.float32(m * np.float32(0.25)) + m))
    assert np.float32(acc * np.float32(1.0 / len(st.mse_S))) == np.float32(st.vq_loss.item())


def test_usages_without_and_with_a_process_group():
    import torch.distributed as tdist
    z, meta = load('a_l2')
    vae = build_vae(meta).eval()
    vae.quantize.ema_vocab_hit_SV.copy_(torch.from_numpy(z['ema']))
    img = torch.from_numpy(z['img'])
    assert not tdist.is_initialized()
    with torch.no_grad():
        alone = vae(img, ret_usages=True)[1]                        # the reference raises here; world size 1 instead
    assert alone == list(z['usages'])
    os.environ.setdefault('GLOO_SOCKET_IFNAME', 'lo')
    tdist.init_process_group('gloo', store=tdist.FileStore(os.path.join(tempfile.mkdtemp(), 'store'), 1), rank=0, world_size=1)
    try:
        with torch.no_grad():
            assert vae(img, ret_usages=True)[1] == alone
    finally:
        tdist.destroy_process_group()


def test_train_mode_with_the_package_dist_flag_runs_the_ema_schedule():
    import torch.distributed as tdist
    from var_amd import dist
    z, meta = load('a_l2')
    vae = build_vae(meta).train()
    q = vae.quantize
    S = len(meta['patch_nums'])
    hit = torch.from_numpy(z['hits_SV']).float()                    # the recorded hit_V of every scale (1 rank: the all-reduce changes nothing)
    f = torch.from_numpy(z['f'])
    os.environ.setdefault('GLOO_SOCKET_IFNAME', 'lo')
    tdist.init_process_group('gloo', store=tdist.FileStore(os.path.join(tempfile.mkdtemp(), 'store'), 1), rank=0, world_size=1)
    dist._state['init'] = True
    try:
        want = q.ema_vocab_hit_SV.clone()
        with torch.no_grad():
            for start in (0, 1, 99, 100, 101):                      # copy_ at 0; 0.9 / 0.1 below 100; 0.99 / 0.01 from 100 on
                q.record_hit = start
                assert not q._forward_on_hip(f)
                q(f)
                rh = start
                for si in range(S):
                    if rh == 0: want[si].copy_(hit[si])
                    elif rh < 100: want[si].mul_(0.9).add_(hit[si].mul(0.1))
                    else: want[si].mul_(0.99).add_(hit[si].mul(0.01))
                    rh += 1
                assert q.record_hit == start + S
                assert torch.equal(q.ema_vocab_hit_SV, want), start
        q.eval(); q.record_hit = 7
        with torch.no_grad():
            q(f)
        assert q.record_hit == 7 and torch.equal(q.ema_vocab_hit_SV, want)         # eval mode: the buffer is only read
    finally:
        dist._state['init'] = False
        tdist.destroy_process_group()


def test_half_input_is_cast_and_cpu_never_takes_hip():
    z, meta = load('a_l2')
    vae = build_vae(meta).eval()
    f = torch.from_numpy(z['f'])
    assert not vae.quantize._forward_on_hip(f) and not vae._forward_on_hip(torch.from_numpy(z['img']))
    with torch.no_grad():
        a = vae.quantize(f.half())
        b = vae.quantize(f.half().float())
    assert a[0].dtype == torch.float32 and torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_new_entry_points():
    """(the argument lists: tests/test_abi_cpu.py, for every declaration of the header)"""
    from var_amd import abi, hip
    hdr = open(os.path.join(ROOT, 'include', 'var_hip.h')).read()
    for name in ('vq_scale_stats_f32', 'vq_loss_combine_f32', 'vq_straight_through_f32'):
        assert name in abi.SIGNATURES_HIP_ONLY and name in hip.lib().fn
    assert hip.vq_stats_blocks(1) == 1 and hip.vq_stats_blocks(4097) == 2 and hip.vq_stats_blocks(1 << 30) == hip.VQ_STATS_MAX_BLOCKS
    assert f'#define VARHIP_VQ_STATS_MAX_BLOCKS {hip.VQ_STATS_MAX_BLOCKS}' in hdr
    # each new entry cites the reference lines it replaces
    sec = hdr[hdr.index('VectorQuantizer2.forward: the tokenizer'):hdr.index('16-bit-input throughput mode')]
    for cite in ('quant.py:77', 'quant.py:95', 'quant.py:98', 'vqvae.py:56-59'):
        assert cite in sec, cite


def test_no_entry_point_of_models_refuses_what_the_reference_runs():
    for path in glob.glob(os.path.join(ROOT, 'var_amd', 'models', '*.py')):
        src = open(path).read()
        if os.path.basename(path) in ('quant.py', 'vqvae.py'):
            assert 'NotImplementedError' not in src, path
    assert 'NotImplementedError' in open(os.path.join(ROOT, 'var_amd', 'models', 'helpers.py')).read()
