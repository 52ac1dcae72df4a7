#!/usr/bin/env python3
"""Timing of VAR as a zero-shot classifier (fork eval_prob.py --mode bayesian, var_analysis.py --cfg) on one MI355X, random-init weights
(detinit seed 0), N images of 256x256, d16:

    new route  VAR.token_scores(gt_tokens, classes, --score, cfg)                  (N x K rows packed into passes of <= --max-rows rows;
               --score log_prob is VAR.token_log_likelihood)
    old route  per image: x = idxBl_to_var_input, VAR.forward(classes, x.expand(K, ...)) [+ one unconditional forward and the CFG combine],
               then the fork's formula on the (K, L, V) logits: log_softmax + gather (log_prob), or sort / softmax / gathers of the
               distance table rows (token_score_torch: group_smoothed, neighbor_max, expected_distance)

both in the same process, alternated, the old one on a stream of its own (each route keeps its own workspace).  With --keep s:m,... the old
route is replaced by

    classify   VAR.classify(gt_tokens, classes, --score, cfg, keep={s: m, ...})   (per-scale pruning; the new route is its unpruned baseline)

and each K reports both routes' ms per image and peak allocation, the class row-tokens the transformer ran (engine.classify_work) against the
unpruned N x K x L, and how often classify's pred equals the unpruned rule argmax (informational: the weights are random).

    python tools/bench_classify.py [--images 16] [--k-large 100] [--cfg 0] [--dtype f32|f16|bf16] [--iters 3] [--keep 4:50,7:10]
                                   [--score log_prob|group_smoothed|neighbor_max|expected_distance] [--group 50] [--threshold T] [--top-k k]

Prints one JSON object: encode ms per image; per K: ms per image and images per second of both routes, their peak allocation increase,
max |delta| of the per-token values; the scoring kernel's time from the library's timing table (family 'sampler', which no other kernel of
the new route uses) and its bytes/s against the 8 TB/s HBM peak."""
import argparse
import contextlib
import io
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from var_amd import detinit, hip      # noqa: E402
from var_amd.models.var import classify_rule, token_score_torch      # noqa: E402

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=16)
    ap.add_argument('--k-large', type=int, default=100)
    ap.add_argument('--cfg', type=float, default=0.0)
    ap.add_argument('--max-rows', type=int, default=64)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--dtype', default='f32', choices=['f32', 'f16', 'bf16'])
    ap.add_argument('--score', default='log_prob', choices=['log_prob', 'group_smoothed', 'neighbor_max', 'expected_distance'])
    ap.add_argument('--group', type=int, default=50)
    ap.add_argument('--threshold', type=float, default=None, help='neighbor_max; default: the median code distance')
    ap.add_argument('--top-k', type=int, default=None, help='expected_distance; default: all codes')
    ap.add_argument('--keep', default=None, help='s:m,s:m,...  time VAR.classify with this pruning schedule instead of the old route')
    a = ap.parse_args()
    keep = None if a.keep is None else {int(k): int(m) for k, m in (item.split(':') for item in a.keep.split(','))}
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    from models import build_vae_var
    pns = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
    with contextlib.redirect_stdout(io.StringIO()):
        vae, var = build_vae_var(device=dev, patch_nums=pns, depth=16, ch=160)
    detinit.fill_module_device_(var, 16, 0, 'var.'); detinit.fill_module_device_(vae, 16, 0, 'vae.')
    var.eval(); vae.eval(); var.cond_drop_rate = 0.0
    var.set_hip_precision(a.dtype)
    N, S = a.images, len(pns)
    g = torch.Generator(device=dev).manual_seed(0)
    img = torch.rand(N, 3, 256, 256, device=dev, generator=g) * 2 - 1
    ev = lambda: torch.cuda.Event(enable_timing=True)
    side = torch.cuda.Stream()

    with torch.inference_mode():
        enc = []
        for it in range(a.iters + 1):
            e0, e1 = ev(), ev()
            e0.record()
            idx = vae.img_to_idxBl(img)
            e1.record(); torch.cuda.synchronize()
            if it: enc.append(e0.elapsed_time(e1))
        gt = torch.cat(idx, 1)
        ratio = torch.tensor([si / (S - 1) for si, pn in enumerate(pns) for _ in range(pn * pn)], device=dev)
        t = a.cfg * ratio.unsqueeze(0).unsqueeze(-1)

        dist = var.engine().code_distance_table() if a.score in ('neighbor_max', 'expected_distance') else None     # built once, outside the timing
        kw, desc = {}, None
        if a.score == 'group_smoothed':
            kw, desc = dict(group=a.group), ('group_smoothed', a.group)
        elif a.score == 'neighbor_max':
            thr = float(dist[:64].median()) if a.threshold is None else a.threshold
            kw, desc = dict(threshold=thr), ('neighbor_max', thr)
        elif a.score == 'expected_distance':
            kw, desc = dict(top_k=a.top_k), ('expected_distance', a.top_k or 0)

        def new_route(classes):
            return var.token_scores(gt, classes, a.score, cfg=a.cfg, max_rows=a.max_rows, **kw)

        def old_route(classes):
            lab = torch.tensor(classes, device=dev)
            out = []
            for i in range(N):
                x = vae.quantize.idxBl_to_var_input([j[i:i + 1] for j in idx])
                logits = var(lab, x.expand(len(classes), -1, -1).contiguous())
                if a.cfg > 0:
                    logits = (1 + t) * logits - t * var(torch.tensor([var.num_classes], device=dev), x)
                if desc is None:
                    lp = torch.nn.functional.log_softmax(logits, dim=-1)
                    out.append(lp.gather(-1, gt[i:i + 1].expand(len(classes), -1).unsqueeze(-1)).squeeze(-1))
                else:
                    out.append(token_score_torch(logits, gt[i], desc, None if dist is None else dist[gt[i]]))
                del logits
            return torch.stack(out)

        def classify_route(classes):
            return var.classify(gt, classes, a.score, cfg=a.cfg, max_rows=a.max_rows, keep=keep, **kw)

        if keep is not None:
            old_route = classify_route

        def timed(fn, classes, stream):
            with torch.cuda.stream(stream):
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                e0, e1 = ev(), ev()
                e0.record()
                r = fn(classes)
                e1.record()
                torch.cuda.synchronize()
                return r, e0.elapsed_time(e1), torch.cuda.max_memory_allocated() - base

        res = dict(images=N, cfg=a.cfg, dtype=a.dtype, max_rows=a.max_rows, score=a.score, score_args=kw, keep=a.keep,
                   encode_ms_per_image=sum(enc) / len(enc) / N)
        for K in (10, a.k_large):
            classes = [(c * 97) % 1000 for c in range(K)]
            ms = {'new': [], 'old': []}
            peak = {'new': 0, 'old': 0}
            timed(new_route, classes, torch.cuda.current_stream()); timed(old_route, classes, side)      # warm-up: weights, workspaces
            for it in range(a.iters):                                                                        # alternated
                ln, tn, pn_ = timed(new_route, classes, torch.cuda.current_stream())
                lo, to, po = timed(old_route, classes, side)
                ms['new'].append(tn); ms['old'].append(to)
                peak['new'] = max(peak['new'], pn_); peak['old'] = max(peak['old'], po)
            best = {k: min(v) for k, v in ms.items()}
            res[f'K{K}'] = dict(
                new_ms_per_image=best['new'] / N, new_images_per_s=1e3 * N / best['new'],
                old_ms_per_image=best['old'] / N, old_images_per_s=1e3 * N / best['old'], speedup=best['old'] / best['new'],
                new_peak_alloc_mb=peak['new'] / 1e6, old_peak_alloc_mb=peak['old'] / 1e6)
            if keep is None:
                res[f'K{K}'].update(max_abs_delta=float((ln - lo).abs().max()), agree_argmax=bool(torch.equal(ln.sum(-1).argmax(-1), lo.sum(-1).argmax(-1))))
            else:                   # 'old' is classify: speedup = unpruned time / classify time
                work = var.engine().classify_work
                ref_pred = classify_rule(ln.cpu().numpy(), [e for _, e in var.begin_ends], [])[0]
                res[f'K{K}'].update(classify_speedup=best['new'] / best['old'], classify_work=work, classify_row_tokens=sum(w for _, _, w in work), unpruned_row_tokens=N * K * var.L,
                                    row_token_ratio=N * K * var.L / sum(w for _, _, w in work),
                                    pred_agrees_with_unpruned=float((lo.pred.cpu().numpy() == ref_pred).mean()))
                # where classify's time goes: every kernel family of one call, from the timing table (events around each launch)
                hip.timing_reset(); hip.timing_enable(True)
                classify_route(classes)
                torch.cuda.synchronize()
                fam = hip.timing_read()
                hip.timing_enable(False)
                res[f'K{K}']['classify_family_ms'] = {k: round(v['ms'], 3) for k, v in fam.items() if v['launches']}
            # the scoring kernel alone, from the timing table (HIP events around each of its launches)
            hip.timing_reset(); hip.timing_enable(True, ['sampler'])
            new_route(classes)
            torch.cuda.synchronize()
            tt = hip.timing_read()['sampler']
            hip.timing_enable(False)
            res[f'K{K}'].update(kernel_ms_per_call=tt['ms'], kernel_launches=tt['launches'], kernel_bytes=tt['bytes'],
                                kernel_TBps=tt['bytes'] / (tt['ms'] * 1e-3) / 1e12 if tt['ms'] > 0 else None,
                                kernel_frac_of_hbm_peak=tt['bytes'] / (tt['ms'] * 1e-3) / HBM_PEAK if tt['ms'] > 0 else None,
                                kernel_share_of_call=tt['ms'] / best['new'])
    print(json.dumps(res))


if __name__ == '__main__':
    main()
