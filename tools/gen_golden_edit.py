#!/usr/bin/env python3
"""Generate tests/golden/edit_*.npz by running the *reference* zero-shot editing loop on CPU: `autoregressive_infer_cfg_with_mask` and
`replace_embedding` of demo_zero_shot_edit.ipynb (cell 2), taken from the notebook at generation time (only data is committed), against the
reference's `models` package, imported unmodified (plus the `torch.Optional` shim of tools/gen_golden.py).  Weights come from var_amd.detinit
through the reference's strict loader, as for the other fixtures; the script runs only where the reference exists.

Cases (tiny random-init configs):
  a  in-painting box, class labels, cfg 1.5, top_k 900, top_p 0.96
  b  out-painting box, label 1000 (the unconditional class)
  c  B = 3, a per-image random binary mask of 7 x 9
  d  more_smooth=True
  e  shared_aln=True, patch_nums (1, 2, 3, 4, 6) (the d36 layout)
  f  a mask whose resize lands on lambda = 1/2: the published 256-pixel schedule (depth 2), a 16 x 16 map with an edge at 8, read at pn = 13

Recorded per case: labels (B,), tokens (B, L) int32 the input tokens, mask (Bm, h, w) fp32, keep (B, L) uint8 the reference's keep maps
(captured from replace_embedding, scales of pn^2 <= 3 included), sampled (B, L) int32 the sampler's tokens and final (B, L) int32 the tokens
after replacement (captured from the codebook lookup; meaningful without more_smooth), f_hat (B, Cvae, P, P), img (B, 3, H, W), noise_head
(S, 8) the first values of each scale's Exp(1) fill (and of the gumbel fill with more_smooth) for the tests to verify their regenerated stream;
meta (JSON): config, seed, cfg, top_k, top_p, more_smooth."""
import contextlib
import io
import json
import os
import sys
import typing

import numpy as np
import torch

torch.Optional = typing.Optional          # shim, see tools/gen_golden.py
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = '/root/reference'
sys.path.insert(0, REF)
sys.path.insert(1, REPO)
GOLD = os.path.join(REPO, 'tests', 'golden')

TINY = dict(depth=2, ch=32, patch_nums=(1, 2, 3, 4, 5), attn_l2_norm=True, shared_aln=False)
SALN = dict(depth=2, ch=32, patch_nums=(1, 2, 3, 4, 6), attn_l2_norm=True, shared_aln=True)
FULL = dict(depth=2, ch=32, patch_nums=(1, 2, 3, 4, 5, 6, 8, 10, 13, 16), attn_l2_norm=True, shared_aln=False)


def notebook_functions():
    """exec the notebook's helper cell (cell 2) and return its namespace"""
    nb = json.load(open(os.path.join(REF, 'demo_zero_shot_edit.ipynb')))
    src = [''.join(c['source']) for c in nb['cells'] if c['cell_type'] == 'code' and 'def replace_embedding' in ''.join(c['source'])]
    assert len(src) == 1
    ns = {}
    exec(compile(src[0], 'demo_zero_shot_edit.ipynb:cell2', 'exec'), ns)
    return ns


def build(cfg):
    from models import build_vae_var
    from var_amd.detinit import fill_module_
    with contextlib.redirect_stdout(io.StringIO()):
        vae, var = build_vae_var(device='cpu', patch_nums=cfg['patch_nums'], depth=cfg['depth'], ch=cfg['ch'], shared_aln=cfg['shared_aln'],
                                 attn_l2_norm=cfg['attn_l2_norm'])
    fill_module_(var, cfg['depth'], 0, 'var.')
    fill_module_(vae, cfg['depth'], 0, 'vae.')
    var.load_state_dict({k: v.clone() for k, v in var.state_dict().items()}, strict=True)
    vae.load_state_dict({k: v.clone() for k, v in vae.state_dict().items()}, strict=True)
    return vae.eval(), var.eval()


def run_case(ns, name, cfg, B, labels, mask, seed, cfg_w, top_k, top_p, more_smooth, img_seed):
    vae, var = build(cfg)
    pns = cfg['patch_nums']
    P = pns[-1]
    g = torch.Generator(); g.manual_seed(img_seed)
    img_in = torch.rand(B, 3, 16 * P, 16 * P, generator=g) * 2 - 1
    with torch.inference_mode():
        toks = vae.img_to_idxBl(img_in)

    keeps, sampled, finals, fhats = [], [], [], []
    orig_replace = ns['replace_embedding']

    def replace(edit_mask, h_BChw, gt_BChw, ph, pw):
        # the keep map replace_embedding computes (recomputed here with its own code, so nothing of it is re-derived)
        Bh = h_BChw.shape[0]
        ones = torch.ones(Bh, 1, ph, pw)
        keeps.append(orig_replace(edit_mask, ones, torch.full_like(ones, 2.0), ph, pw).eq(2.0).view(Bh, -1).to(torch.uint8))
        return orig_replace(edit_mask, h_BChw, gt_BChw, ph, pw)
    ns['replace_embedding'] = replace
    orig_sample = ns['sample_with_top_k_top_p_']

    def sample(*a, **k):
        r = orig_sample(*a, **k)
        sampled.append(r[:, :, 0].clone())
        return r
    ns['sample_with_top_k_top_p_'] = sample
    quant = vae.quantize
    orig_next = quant.get_next_autoregressive_input

    def get_next(si, SN, f_hat, h):
        f, nxt = orig_next(si, SN, f_hat, h)
        fhats.append(f.detach().clone())
        return f, nxt
    quant.get_next_autoregressive_input = get_next
    with torch.inference_mode():
        out = ns['autoregressive_infer_cfg_with_mask'](var, B=B, label_B=torch.tensor(labels), g_seed=seed, cfg=cfg_w, top_k=top_k, top_p=top_p,
                                                        more_smooth=more_smooth, input_img_tokens=toks, edit_mask=mask)
    ns['replace_embedding'] = orig_replace
    ns['sample_with_top_k_top_p_'] = orig_sample
    keep = torch.cat(keeps, 1)
    tok = torch.cat(toks, 1)
    samp = torch.cat(sampled, 1)
    final = torch.where(keep.bool(), tok, samp)

    gg = torch.Generator(); gg.manual_seed(seed)
    heads = []
    V = var.V
    for pn in pns:
        a = torch.empty(B * pn * pn, V).exponential_(1, generator=gg)
        hd = a.view(-1)[:4].numpy()
        if more_smooth:
            b = torch.empty(B, pn * pn, V).exponential_(generator=gg)
            hd = np.concatenate([hd, b.view(-1)[:4].numpy()])
        else:
            hd = np.concatenate([hd, a.view(-1)[4:8].numpy()])
        heads.append(hd)
    meta = dict(cfg, B=B, V=V, labels=list(labels), seed=seed, cfg=cfg_w, top_k=top_k, top_p=top_p, more_smooth=more_smooth, img_seed=img_seed)
    meta['patch_nums'] = list(pns)
    rec = dict(labels=np.array(labels, np.int64), tokens=tok.numpy().astype(np.int32), mask=mask.float().reshape(-1, *mask.shape[-2:]).numpy(),
               keep=keep.numpy(), sampled=samp.numpy().astype(np.int32), final=final.numpy().astype(np.int32), f_hat=fhats[-1].numpy(),
               img=out.float().numpy(), noise_head=np.stack(heads).astype(np.float32), meta=np.array(json.dumps(meta)))
    path = os.path.join(GOLD, f'edit_{name}.npz')
    np.savez_compressed(path, **rec)
    print(f'[gen_golden_edit] {name}: kept {int(keep.sum())} / {keep.numel()}, img mean {out.mean():.4f}, {os.path.getsize(path)} bytes', flush=True)


def main():
    if not os.path.isdir(os.path.join(REF, 'models')):
        sys.exit('gen_golden_edit: the reference is not on this machine')
    ns = notebook_functions()
    gem = ns['get_edit_mask']
    P = TINY['patch_nums'][-1]
    run_case(ns, 'a_inpaint', TINY, 2, (980, 437), gem(TINY['patch_nums'], 0.1, 0.1, 0.8, 0.8, 'cpu', inpainting=True), 1, 1.5, 900, 0.96, False, 21)
    run_case(ns, 'b_outpaint', TINY, 2, (1000, 1000), gem(TINY['patch_nums'], 0.2, 0.3, 0.7, 0.9, 'cpu', inpainting=False), 2, 1.5, 900, 0.96,
             False, 22)
    g = torch.Generator(); g.manual_seed(23)
    run_case(ns, 'c_b3_7x9', TINY, 3, (0, 500, 999), (torch.rand(3, 7, 9, generator=g) < 0.5).float(), 3, 3.0, 600, 0.5, False, 23)
    run_case(ns, 'd_more_smooth', TINY, 2, (3, 7), gem(TINY['patch_nums'], 0.1, 0.1, 0.8, 0.8, 'cpu', inpainting=True), 4, 1.5, 900, 0.96, True, 24)
    Ps = SALN['patch_nums'][-1]
    run_case(ns, 'e_saln', SALN, 2, (1, 999), gem(SALN['patch_nums'], 0.25, 0.0, 0.75, 0.5, 'cpu', inpainting=True), 5, 1.5, 900, 0.96, False, 25)
    # a 16 x 16 map with a box edge at row / column 8: resized to pn = 13 the source coordinate of d = 6 is 7.5 (+1 ulp when fused)
    half = torch.zeros(16, 16); half[8:, :] = 1; half[:, 8:] = 1
    run_case(ns, 'f_half', FULL, 1, (11,), half, 6, 1.5, 900, 0.96, False, 26)
    assert P == 5 and Ps == 6


if __name__ == '__main__':
    main()
