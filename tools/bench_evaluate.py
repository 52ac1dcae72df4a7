#!/usr/bin/env python3
"""Timing of the trainer's validation pass (reference trainer.py:54-84 eval_ep, :126-156 the logging block) on one MI355X, random-init weights
(detinit seed 0), d16, B images of 256x256 given as tokens, in f32 and bf16:

    new route  r = VAR.evaluate(gt, label, max_rows=B); r.L_mean, r.L_tail, r.acc_mean, r.acc_tail, r.per_scale(), r.z_voc_usage
    old route  the same numbers as eval_ep and the tensorboard block compute them: logits = var(label, x), F.cross_entropy on all tokens and
               on the last scale, the two argmax comparisons, the per-scale loop, the bincount of the predictions

both in the same process, alternated, the old one on a stream of its own (each route keeps its own workspace); every timed call ends in a
device-to-host transfer of its numbers.  The teacher-forcing input (idxBl_to_var_input) is inside both.

    python tools/bench_evaluate.py [--images 64] [--iters 5] [--warmup 2] [--out profiles/evaluate_bench.json]

Prints one JSON object (and writes it to --out): per dtype the median, min and max ms per call of both routes, images per second at the
median, the peak allocation increase of a call (torch.cuda.max_memory_allocated), max |delta| of the numbers between the routes, and the
evaluation kernels' own time from the library's timing table (family 'sampler', which nothing else in the new route uses) with their bytes/s
against the 8 TB/s HBM peak."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from var_amd import detinit, hip      # noqa: E402

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    from models import build_vae_var
    pns = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
    with contextlib.redirect_stdout(io.StringIO()):
        vae, var = build_vae_var(device=dev, patch_nums=pns, depth=16, ch=160)
    detinit.fill_module_device_(var, 16, 0, 'var.'); detinit.fill_module_device_(vae, 16, 0, 'vae.')
    var.eval(); vae.eval(); var.cond_drop_rate = 0.0
    B, V, L = a.images, var.V, var.L
    g = torch.Generator(device=dev).manual_seed(0)
    gt = torch.randint(0, V, (B, L), device=dev, generator=g)
    lab = torch.randint(0, 1000, (B,), device=dev, generator=g)
    last = pns[-1] ** 2
    F = torch.nn.functional
    ev = lambda: torch.cuda.Event(enable_timing=True)
    side = torch.cuda.Stream()

    def new_route():
        r = var.evaluate(gt, lab, max_rows=B)
        return dict(L_mean=r.L_mean, L_tail=r.L_tail, acc_mean=r.acc_mean, acc_tail=r.acc_tail, z_voc_usage=r.z_voc_usage, **r.per_scale())

    def old_route():
        idx = [gt[:, b:e] for b, e in var.begin_ends]
        logits = var(lab, vae.quantize.idxBl_to_var_input(idx))
        out = dict(L_mean=F.cross_entropy(logits.view(-1, V), gt.view(-1)),
                   L_tail=F.cross_entropy(logits[:, -last:].reshape(-1, V), gt[:, -last:].reshape(-1)),
                   acc_mean=(logits.argmax(dim=-1) == gt).sum() * (100 / L / B),
                   acc_tail=(logits[:, -last:].argmax(dim=-1) == gt[:, -last:]).sum() * (100 / last / B))
        pred = logits.argmax(dim=-1)
        p = pred.view(-1).bincount(minlength=V).float()
        p /= p.sum()
        out['z_voc_usage'] = (p > 0.001 / V).float().mean() * 100
        for (b, e), pn in zip(var.begin_ends, pns):
            z, tar = logits[:, b:e].reshape(-1, V), gt[:, b:e].reshape(-1)
            out[f'acc_{16 * pn}'] = (z.argmax(dim=-1) == tar).float().mean() * 100
            out[f'L_{16 * pn}'] = F.cross_entropy(z, tar)
        return {k: float(v) for k, v in out.items()}

    def timed(fn, stream):
        with torch.cuda.stream(stream):
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            e0, e1 = ev(), ev()
            e0.record()
            r = fn()
            e1.record()
            torch.cuda.synchronize()
            return r, e0.elapsed_time(e1), torch.cuda.max_memory_allocated() - base

    res = dict(images=B, depth=16, L=L, V=V, iters=a.iters, warmup=a.warmup, full_logits_mb=B * L * V * 4 / 1e6)
    with torch.inference_mode():
        for dtype in ('f32', 'bf16'):
            var.set_hip_precision(dtype)
            for _ in range(a.warmup):
                timed(new_route, torch.cuda.current_stream()); timed(old_route, side)
            ms, peak = {'new': [], 'old': []}, {'new': 0, 'old': 0}
            for _ in range(a.iters):                                                                         # alternated
                rn, tn, pn_ = timed(new_route, torch.cuda.current_stream())
                ro, to, po = timed(old_route, side)
                ms['new'].append(tn); ms['old'].append(to)
                peak['new'] = max(peak['new'], pn_); peak['old'] = max(peak['old'], po)
            d = {}
            for k in ('new', 'old'):
                med = statistics.median(ms[k])
                d[k] = dict(ms_median=med, ms_min=min(ms[k]), ms_max=max(ms[k]), images_per_s=1e3 * B / med, peak_alloc_mb=peak[k] / 1e6)
            d['speedup_at_median'] = d['old']['ms_median'] / d['new']['ms_median']
            d['max_abs_delta'] = max(abs(rn[k] - ro[k]) for k in rn)
            hip.timing_reset(); hip.timing_enable(True, ['sampler'])
            new_route()
            torch.cuda.synchronize()
            tt = hip.timing_read()['sampler']
            hip.timing_enable(False)
            d['kernel'] = dict(ms_per_call=tt['ms'], launches=tt['launches'], bytes=tt['bytes'],
                               TBps=tt['bytes'] / (tt['ms'] * 1e-3) / 1e12 if tt['ms'] > 0 else None,
                               frac_of_hbm_peak=tt['bytes'] / (tt['ms'] * 1e-3) / HBM_PEAK if tt['ms'] > 0 else None,
                               share_of_call=tt['ms'] / d['new']['ms_median'])
            res[dtype] = d
        var.set_hip_precision('f32')
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
