#!/usr/bin/env python3
"""Generate tests/golden/generative_t_pn12345.npz by running the *reference* generative classifier (eval_prob.py:466-516, `--mode gen`)
on CPU.  Follows tools/gen_golden.py: the reference's `models` package is imported unmodified (plus the same `torch.Optional` shim), its
weights come from var_amd.detinit through the reference's own strict loader, and the script runs only where the reference exists.

Per image, class set, `cfg` in {0, 4}, `c` (--Clayer) in {1, 2} and feature in {vae_post, vae_fhat} it computes exactly what eval_prob.py
does: gt tokens = vae.img_to_idxBl(img), mask[:, cumsum(pn^2)[c]:] = 0, var.inpainting(gt.repeat(K), mask.repeat(K), cfg, top_k=1, top_p=0,
label, g_seed), then -mean|feat(img) - feat(rec)| with feat = img_to_post or img_to_fhat(...)[-1] (the reconstruction in [0, 1], the input in
[-1, 1]), and pred = argmax.  Every greedy position's guided logits are checked for an exact tie at the row maximum (`ties` records the
count: the fixture is only meaningful for the tie-free greedy rule when it is 0).

Recorded: img (N,3,80,80), labels (K,), gt (N, L) the input tokens; per setting `{feat}_cfg{cfg}_c{c}`: tokens (N, K, L) int32 (the
reconstruction's tokens), f_in (N, Cvae, 5, 5), f_rec (N, K, Cvae, 5, 5), score (N, K) fp32, pred (N,) int64; meta (JSON)."""
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
CFG = dict(depth=2, ch=32, patch_nums=(1, 2, 3, 4, 5), attn_l2_norm=True, shared_aln=False)
LABELS = (980, 437, 3, 1000, 7, 512)
CFGS = (0.0, 4.0)
CLAYERS = (1, 2)
FEATURES = ('vae_post', 'vae_fhat')
IMG_SEED, G_SEED = 41, 0


def main():
    if not os.path.isdir(os.path.join(REF, 'models')):
        sys.exit('gen_golden_generative: the reference is not on this machine')
    import models.var as ref_var
    from models import build_vae_var
    from var_amd.detinit import fill_module_
    with contextlib.redirect_stdout(io.StringIO()):
        vae, var = build_vae_var(device='cpu', patch_nums=CFG['patch_nums'], depth=CFG['depth'], ch=CFG['ch'],
                                 shared_aln=CFG['shared_aln'], attn_l2_norm=CFG['attn_l2_norm'])
    fill_module_(var, CFG['depth'], 0, 'var.')
    fill_module_(vae, CFG['depth'], 0, 'vae.')
    var.load_state_dict({k: v.clone() for k, v in var.state_dict().items()}, strict=True)
    vae.load_state_dict({k: v.clone() for k, v in vae.state_dict().items()}, strict=True)
    vae.eval(); var.eval()

    ties = [0]
    orig = ref_var.sample_with_top_k_top_p_

    def counting(logits_BlV, top_k=0, top_p=0.0, rng=None, num_samples=1):
        assert top_k == 1
        mx = logits_BlV.amax(-1, keepdim=True)
        ties[0] += int(((logits_BlV == mx).sum(-1) > 1).sum())
        return orig(logits_BlV, top_k=top_k, top_p=top_p, rng=rng, num_samples=num_samples)
    ref_var.sample_with_top_k_top_p_ = counting

    P = CFG['patch_nums'][-1]
    g = torch.Generator(); g.manual_seed(IMG_SEED)
    img = torch.rand(2, 3, 16 * P, 16 * P, generator=g) * 2 - 1
    N, K = img.shape[0], len(LABELS)
    cumsum = np.cumsum([p * p for p in CFG['patch_nums']])
    label_B = torch.tensor(LABELS)
    rec = dict(img=img.numpy(), labels=np.array(LABELS, dtype=np.int64))
    with torch.inference_mode():
        gt_all = torch.cat(vae.img_to_idxBl(img), dim=1)
        rec['gt'] = gt_all.numpy().astype(np.int32)
        for cfg in CFGS:
            for c in CLAYERS:
                outs = []
                for n in range(N):
                    gt_tokens = gt_all[n:n + 1]
                    mask = torch.ones_like(gt_tokens)
                    mask[:, cumsum[c]:] = 0
                    finals = []
                    hk = vae.quantize.embedding.register_forward_hook(lambda m, inp, out: finals.append(inp[0].detach().clone()))
                    out = var.inpainting(gt_tokens.repeat(K, 1), mask.repeat(K, 1).bool(), cfg=cfg, top_k=1, top_p=0, label=label_B, g_seed=G_SEED)
                    hk.remove()
                    outs.append((out, torch.cat(finals, 1)))
                for feat in FEATURES:
                    key = f'{feat}_cfg{int(cfg)}_c{c}'
                    toks, f_in, f_rec, score = [], [], [], []
                    for n in range(N):
                        out, tk = outs[n]
                        if feat == 'vae_fhat':
                            fi, fr = vae.img_to_fhat(img[n:n + 1])[-1], vae.img_to_fhat(out)[-1]
                        else:
                            fi, fr = vae.img_to_post(img[n:n + 1]), vae.img_to_post(out)
                        l1 = torch.abs(fi.view(1, -1) - fr.view(K, -1)).mean(dim=-1)
                        toks.append(tk.numpy().astype(np.int32)); f_in.append(fi[0].numpy()); f_rec.append(fr.numpy()); score.append((-l1).numpy())
                    score = np.stack(score).astype(np.float32)
                    rec[f'{key}_tokens'] = np.stack(toks)
                    rec[f'{key}_f_in'] = np.stack(f_in)
                    rec[f'{key}_f_rec'] = np.stack(f_rec)
                    rec[f'{key}_score'] = score
                    rec[f'{key}_pred'] = score.argmax(-1).astype(np.int64)
                    print(f'[gen_golden_generative] {key}: pred {rec[key + "_pred"].tolist()}', flush=True)
    meta = dict(CFG, labels=list(LABELS), cfgs=list(CFGS), clayers=list(CLAYERS), features=list(FEATURES), img_seed=IMG_SEED, g_seed=G_SEED,
                ties=ties[0])
    rec['meta'] = np.array(json.dumps(meta))
    if ties[0]:
        sys.exit(f'gen_golden_generative: {ties[0]} greedy rows with an exact tie at the maximum')
    path = os.path.join(GOLD, 'generative_t_pn12345.npz')
    np.savez_compressed(path, **rec)
    print(f'[gen_golden_generative] wrote {path} ({os.path.getsize(path)} bytes), ties {ties[0]}', flush=True)


if __name__ == '__main__':
    main()
