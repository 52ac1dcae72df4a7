#!/usr/bin/env python3
"""Timing of zero-shot editing on one MI355X, random-init weights (detinit seed 0): VAR.autoregressive_infer_cfg_with_mask (an in-painting
box, get_edit_mask(0.1, 0.1, 0.8, 0.8)) against VAR.autoregressive_infer_cfg at the same seed, per precision, for

    d16       256 x 256, B = 64      patch_nums (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
    d36-saln  512 x 512, B = 8       patch_nums (1, 2, 3, 4, 6, 9, 13, 18, 24, 32), shared AdaLN

and, informational, the "old route": the editing notebook's loop run on this package's eager modules (SDPA blocks with torch.cat KV caches,
the PyTorch quantizer step, F.interpolate masks; only the decoder reaches HIP), f32, at --old-b rows.  The output check runs the old route and
the engine on the same seeded noise-free input (top_k = 1, so both pick the argmax) and reports the largest pixel difference.

    python tools/bench_edit.py [--configs d16,d36] [--precisions f32,f16,bf16] [--iters 3] [--old-b 8] [--no-old]

Prints one JSON object: per config and precision images/s of both calls and their ratio, and the old route's images/s and check."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from var_amd import detinit      # noqa: E402

CONFIGS = {'d16': dict(depth=16, shared_aln=False, patch_nums=(1, 2, 3, 4, 5, 6, 8, 10, 13, 16), B=64),
           'd36': dict(depth=36, shared_aln=True, patch_nums=(1, 2, 3, 4, 6, 9, 13, 18, 24, 32), B=8)}


@torch.no_grad()
def eager_edit(var, vae, B, label_B, cfg, tokens, mask):
    """the masked AR loop on the eager nn.Modules (greedy, for the output check and the old route's timing)"""
    quant = vae.quantize
    cond = var.class_emb(torch.cat((label_B, torch.full_like(label_B, var.num_classes))))
    lvl_pos = var.lvl_embed(var.lvl_1L) + var.pos_1LC
    x = cond.unsqueeze(1).expand(2 * B, var.first_l, -1) + var.pos_start.expand(2 * B, var.first_l, -1) + lvl_pos[:, :var.first_l]
    P = var.patch_nums[-1]
    f_hat = cond.new_zeros(B, var.Cvae, P, P)
    cond_g = var.shared_ada_lin(cond)
    for b in var.blocks: b.attn.kv_caching(True)
    cur = 0
    S = len(var.patch_nums)
    for si, pn in enumerate(var.patch_nums):
        t = cfg * si / (S - 1)
        h = x
        for b in var.blocks:
            h = b(x=h, cond_BD=cond_g, attn_bias=None)
        lg = var.get_logits(h, cond)
        lg = (1 + t) * lg[:B] - t * lg[B:]
        idx = lg.argmax(-1)
        keep = F.interpolate(mask[:, None], size=(pn, pn), mode='bilinear', align_corners=False) > 0.5
        if pn * pn <= 3: keep[:] = True
        idx = torch.where(keep.view(B, -1), tokens[:, cur:cur + pn * pn], idx)
        cur += pn * pn
        hB = quant.embedding(idx).transpose(1, 2).reshape(B, var.Cvae, pn, pn)
        f_hat, nxt = quant.get_next_autoregressive_input(si, S, f_hat, hB)
        if si != S - 1:
            nxt = nxt.view(B, var.Cvae, -1).transpose(1, 2)
            x = (var.word_embed(nxt) + lvl_pos[:, cur:cur + var.patch_nums[si + 1] ** 2]).repeat(2, 1, 1)
    for b in var.blocks: b.attn.kv_caching(False)
    return vae.fhat_to_img(f_hat).add_(1).mul_(0.5)


def timed(fn, iters):
    fn(); torch.cuda.synchronize()
    best = float('inf')
    for _ in range(iters):
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', default='d16,d36')
    ap.add_argument('--precisions', default='f32,f16,bf16')
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--old-b', type=int, default=8)
    ap.add_argument('--no-old', action='store_true')
    a = ap.parse_args()
    from models import build_vae_var
    from models.var import get_edit_mask
    res = {}
    for name in a.configs.split(','):
        c = CONFIGS[name]
        pns, B = c['patch_nums'], c['B']
        with contextlib.redirect_stdout(io.StringIO()):
            vae, var = build_vae_var(device='cuda', patch_nums=pns, depth=c['depth'], ch=160, shared_aln=c['shared_aln'])
        detinit.fill_module_device_(var, c['depth'], 0, 'var.'); detinit.fill_module_device_(vae, c['depth'], 0, 'vae.')
        var.eval(); vae.eval()
        g = torch.Generator(device='cuda').manual_seed(0)
        img = torch.rand(1, 3, 16 * pns[-1], 16 * pns[-1], device='cuda', generator=g) * 2 - 1
        with torch.inference_mode():
            toks = vae.img_to_idxBl(img)
        mask = get_edit_mask(pns, 0.1, 0.1, 0.8, 0.8, 'cuda', inpainting=True)
        labels = torch.arange(B, device='cuda') * 97 % 1000
        kw = dict(cfg=1.5, top_k=900, top_p=0.96, g_seed=0)
        r = {}
        for prec in a.precisions.split(','):
            var.set_hip_precision(prec)
            t_edit = timed(lambda: var.autoregressive_infer_cfg_with_mask(B, labels, input_img_tokens=toks, edit_mask=mask, **kw), a.iters)
            t_plain = timed(lambda: var.autoregressive_infer_cfg(B, labels, **kw), a.iters)
            r[prec] = dict(edit_img_s=round(B / t_edit, 2), plain_img_s=round(B / t_plain, 2), edit_over_plain_time=round(t_edit / t_plain, 4))
            print(f'[bench_edit] {name} {prec}: edit {B / t_edit:.2f} img/s, plain {B / t_plain:.2f} img/s', flush=True)
        var.set_hip_precision('f32')
        if not a.no_old:
            ob = min(a.old_b, B)
            tk = torch.cat(toks, 1).expand(ob, -1).contiguous()
            mk = mask[None].expand(ob, -1, -1).contiguous()
            lab = labels[:ob]
            t_old = timed(lambda: eager_edit(var, vae, ob, lab, 1.5, tk, mk), 1)
            old = eager_edit(var, vae, ob, lab, 1.5, tk, mk)
            new = var.autoregressive_infer_cfg_with_mask(ob, lab, cfg=1.5, top_k=1, top_p=0.0, g_seed=0, input_img_tokens=tk, edit_mask=mask)
            r['old_route_f32'] = dict(B=ob, img_s=round(ob / t_old, 3), max_abs_diff_vs_engine_top_k1=float((old - new).abs().max()))
            print(f'[bench_edit] {name} old route (eager, f32, B={ob}): {ob / t_old:.3f} img/s, |old - engine| max {r["old_route_f32"]["max_abs_diff_vs_engine_top_k1"]:.3g}',
                  flush=True)
        res[name] = r
        del var, vae
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
