#!/usr/bin/env python3
"""Generate tests/golden/vaefwd_*.npz by running the *reference* `VQVAE.forward` (models/vqvae.py:56-59, models/quant.py:52-104) on the CPU,
against the reference's `models` package imported unmodified.  Weights come from var_amd.detinit through the reference's strict loader, as for
the other fixtures; the script runs only where the reference exists.  The reference's forward calls torch.distributed.get_world_size()
unconditionally, so a 1-rank gloo group over a file store (no network) is created first.

Cases (ch 32, 4096 codes of 32 channels):
  a_l2      L2 quantizer, patch_nums (1, 2, 3, 4), B = 2
  b_znorm   using_znorm=True
  c_qsr0    share_quant_resi=0 (one Phi per scale)
  c_qsr1    share_quant_resi=1 (one Phi for all)
  d_b3      B = 3, patch_nums (1, 2, 3, 4, 5)
  e_grad    train mode, requires_grad on, loss = vq_loss + rec.square().mean(); gradients of the codebook, the first Phi conv,
            quant_conv.weight and encoder.conv_in.weight

`ema_vocab_hit_SV` is set to a deterministic pattern that straddles the usage margin before the call (else every usage is 0.0).

Recorded per case: img, ema, f, idx_s{si}, hits_SV, mse_S, vq_loss, usages, f_hat_st, rec, gap_s{si} (per row: best vs runner-up of the
distance / similarity the reference's own argmin / argmax saw), gap_min, meta (JSON).  An input whose gap_min is below what the input of the
existing encode fixture (encode_t_pn12345.npz) exhibits under the same measurement is rejected and the next image seed is tried: the GPU
comparison demands identical tokens, and the reference alone must clear that bar on the inputs chosen."""
import contextlib
import io
import json
import os
import sys
import tempfile
import typing

import numpy as np
import torch
import torch.distributed as tdist

torch.Optional = typing.Optional          # shim, see tools/gen_golden.py
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = '/root/reference'
sys.path.insert(0, REF)
sys.path.insert(1, REPO)
GOLD = os.path.join(REPO, 'tests', 'golden')
DEPTH = 2                                 # detinit's depth argument (the VAE rules do not use it)


def ema_pattern(S, V, margin):
    """(S, V) fp32 straddling `margin`: scale si has about max(0, 1 - 1 / (0.8 + 0.4 si)) of its codes at or above it"""
    v = np.arange(V, dtype=np.int64)[None, :]
    si = np.arange(S, dtype=np.int64)[:, None]
    r = ((v * 37 + si * 101) % 1000).astype(np.float64) / 1000.0
    return (margin * r * (0.8 + 0.4 * si)).astype(np.float32)


@contextlib.contextmanager
def record_gaps(store):
    """the reference picks tokens with torch.argmin (L2) / torch.argmax (cosine): record best vs runner-up of what it passes"""
    amin, amax = torch.argmin, torch.argmax

    def wrap(fn, largest):
        def f(x, *a, **k):
            if x.dim() == 2 and x.shape[1] > 1:
                t = torch.topk(x.detach().double(), 2, dim=1, largest=largest).values
                store.append((t[:, 0] - t[:, 1]).abs().numpy())
            return fn(x, *a, **k)
        return f
    torch.argmin, torch.argmax = wrap(amin, False), wrap(amax, True)
    try:
        yield
    finally:
        torch.argmin, torch.argmax = amin, amax


def build(cfg, test_mode=True):
    from models.vqvae import VQVAE
    from var_amd.detinit import fill_module_
    vae = VQVAE(vocab_size=4096, z_channels=32, ch=cfg['ch'], test_mode=test_mode, share_quant_resi=cfg['share_quant_resi'],
                v_patch_nums=tuple(cfg['patch_nums']), using_znorm=cfg['using_znorm'])
    fill_module_(vae, DEPTH, 0, 'vae.')
    vae.load_state_dict({k: v.clone() for k, v in vae.state_dict().items()}, strict=True)
    return vae


def encode_fixture_gap():
    """gap_min of the existing encode fixture's input, measured the same way on the reference"""
    z = np.load(os.path.join(GOLD, 'encode_t_pn12345.npz'))
    meta = json.loads(str(z['meta']))
    vae = build(dict(ch=meta['ch'], share_quant_resi=4, patch_nums=meta['patch_nums'], using_znorm=False)).eval()
    gaps = []
    with record_gaps(gaps), torch.inference_mode():
        vae.img_to_idxBl(torch.from_numpy(z['img']))
    return float(min(g.min() for g in gaps))


def run_case(name, cfg, B, img_seed, floor, grad=False):
    pns = tuple(cfg['patch_nums'])
    S, P = len(pns), pns[-1]
    while True:
        vae = build(cfg, test_mode=not grad)
        vae.train() if grad else vae.eval()
        g = torch.Generator(); g.manual_seed(img_seed)
        img = torch.rand(B, 3, 16 * P, 16 * P, generator=g) * 2 - 1
        margin = 1 * (B * P * P) / 4096 * 0.08
        ema = ema_pattern(S, 4096, margin)
        vae.quantize.ema_vocab_hit_SV.copy_(torch.from_numpy(ema))
        gaps, idxs = [], []
        emb = vae.quantize.embedding
        hook = emb.register_forward_hook(lambda m, a, o: idxs.append(a[0].detach().reshape(B, -1).clone()))
        with record_gaps(gaps), (contextlib.nullcontext() if grad else torch.no_grad()):
            f = vae.quant_conv(vae.encoder(img))
            rec, usages, vq_loss = vae(img, ret_usages=True)
            f_hat_st, _, vq2 = vae.quantize(f, ret_usages=False)
        hook.remove()
        gaps, idxs = gaps[:S], idxs[:S]                       # (the second quantize call repeats them)
        assert float(vq2) == float(vq_loss)
        # znorm: the reference compares cosines of unit vectors; |a - b|^2 = 2 - 2 cos puts its gap on the L2 scale of unit vectors
        gap_min = min(float(x.min()) for x in gaps) * (2.0 if cfg['using_znorm'] else 1.0)
        if gap_min >= floor:
            break
        print(f'[gen_golden_vae_forward] {name}: image seed {img_seed} has gap_min {gap_min:.3e} < {floor:.3e}: next seed', flush=True)
        img_seed += 1000
    rec_d = dict(img=img.numpy(), ema=ema, f=f.detach().numpy(), f_hat_st=f_hat_st.detach().numpy(), rec=rec.detach().numpy(),
                 vq_loss=np.float32(vq_loss.item()), usages=np.array(usages, np.float64), gap_min=np.float64(gap_min))
    # per-scale quantities the reference does not return: restated from its own outputs (tokens captured at its embedding lookup; f_hat after
    # each scale from its own f_to_idxBl_or_fhat, which runs the same loop)
    with torch.no_grad():
        fhs = vae.quantize.f_to_idxBl_or_fhat(f.detach(), to_fhat=True)
    mse = [torch.nn.functional.mse_loss(fh, f.detach()) for fh in fhs]
    seq = 0.0
    for m in mse:
        seq += m.clone().mul_(vae.quantize.beta) + m
    seq *= 1. / S
    assert float(seq) == float(vq_loss), (float(seq), float(vq_loss))          # the per-scale values ARE what the reference's loss summed
    rec_d['mse_S'] = np.array([m.item() for m in mse], np.float32)
    rec_d['hits_SV'] = np.stack([np.bincount(i.numpy().reshape(-1), minlength=4096) for i in idxs]).astype(np.int64)
    for si in range(S):
        rec_d[f'idx_s{si}'] = idxs[si].numpy().astype(np.int32)
        rec_d[f'gap_s{si}'] = gaps[si].astype(np.float32)
    meta = dict(cfg, B=B, V=4096, Cvae=32, img_seed=img_seed, beta=vae.quantize.beta, grad=grad, margin=margin, gap_floor=floor)
    meta['patch_nums'] = list(pns)
    if grad:
        loss = vq_loss + rec.square().mean()
        loss.backward()
        names = ['quantize.embedding.weight', 'quantize.quant_resi.qresi_ls.0.weight', 'quant_conv.weight', 'encoder.conv_in.weight']
        params = dict(vae.named_parameters())
        for n in names:
            rec_d['grad.' + n] = params[n].grad.numpy()
        rec_d['loss'] = np.float32(loss.item())
        meta['grad_names'] = names
    rec_d['meta'] = np.array(json.dumps(meta))
    path = os.path.join(GOLD, f'vaefwd_{name}.npz')
    np.savez_compressed(path, **rec_d)
    assert os.path.getsize(path) <= 1 << 20, path
    print(f'[gen_golden_vae_forward] {name}: vq_loss {float(vq_loss):.6f} usages {[round(u, 2) for u in usages]} rec in [{float(rec.min()):.2f}, '
          f'{float(rec.max()):.2f}] gap_min {gap_min:.3e} {os.path.getsize(path)} bytes', flush=True)


def main():
    if not os.path.isdir(os.path.join(REF, 'models')):
        sys.exit('gen_golden_vae_forward: the reference is not on this machine')
    store = os.path.join(tempfile.mkdtemp(), 'store')
    os.environ.setdefault('GLOO_SOCKET_IFNAME', 'lo')          # one rank: the loopback interface is all gloo needs
    tdist.init_process_group('gloo', store=tdist.FileStore(store, 1), rank=0, world_size=1)
    with contextlib.redirect_stdout(io.StringIO()):
        floor = encode_fixture_gap()
    print(f'[gen_golden_vae_forward] gap floor (encode_t_pn12345.npz input): {floor:.3e}', flush=True)
    base = dict(ch=32, share_quant_resi=4, patch_nums=(1, 2, 3, 4), using_znorm=False)
    run_case('a_l2', base, 2, 31, floor)
    run_case('b_znorm', dict(base, using_znorm=True), 2, 32, floor)
    run_case('c_qsr0', dict(base, share_quant_resi=0), 2, 33, floor)
    run_case('c_qsr1', dict(base, share_quant_resi=1), 2, 34, floor)
    run_case('d_b3', dict(base, patch_nums=(1, 2, 3, 4, 5)), 3, 35, floor)
    run_case('e_grad', base, 2, 36, floor, grad=True)
    tdist.destroy_process_group()


if __name__ == '__main__':
    main()
