#!/usr/bin/env python3
"""Timing of VAR.sample_composed on one MI355X, random-init weights (detinit seed 0), VAR-d16 256 x 256, B = 8, cfg 1.5, top-k 900, top-p 0.96,
per precision (2 warm-up rounds, --iters (>= 5) timed rounds, median of HIP-event times; the variants of a comparison alternate call by
call inside a round, so they see the same machine):
  (a) sample_composed with K = 1, w = 1 against VAR.autoregressive_infer_cfg_per_image_scored, which computes the same bits; with
      --parent-root DIR the per-image scored call of that (built) checkout is timed too, in fresh processes alternating with this checkout's
      (parent, this, parent, this): the two runs per checkout give the process-to-process spread, the min..max of a run the spread inside it;
  (b) K = 2 and K = 4 (K + 1 transformer rows per image instead of 2) against (a);
  (c) varhip_mix_sample_rows_f32 at G = 2, 3, 5 against varhip_cfg_sample_rows_f32 on the (B, l, V) of the last scale: --reps launches
      between one pair of events, per launch; bytes = the G logit rows + noise read and the filtered (and guided) rows written.

    python tools/bench_compose.py [--precisions f32,bf16] [--iters 7] [--B 8] [--parent-root DIR] [--out profiles/compose_bench.json]
    python tools/bench_compose.py --scored-only [--root OTHER_CHECKOUT]      # the per-image scored call alone (what --parent-root spawns)

Informational: no threshold is attached to any of these numbers.  Prints one JSON object (and writes it to --out)."""
import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys

PNS = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
KW = dict(cfg=1.5, top_k=900, top_p=0.96)
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def summary(ms: list) -> dict:
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), samples=[round(x, 3) for x in ms])


def rounds_ms(fns: dict, warmup: int, iters: int) -> dict:
    """every round runs each variant once, in the dict's order, each between its own pair of events -> {name: [ms per round]}"""
    import torch
    out = {k: [] for k in fns}
    for r in range(warmup + iters):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            torch.cuda.synchronize()
            if r >= warmup:
                out[name].append(a.elapsed_time(b))
    return out


def build_model(root: str):
    import torch  # noqa: F401
    sys.path.insert(0, os.path.abspath(root))
    from models import build_vae_var
    from var_amd import detinit
    with contextlib.redirect_stdout(io.StringIO()):
        vae, var = build_vae_var(device='cuda', patch_nums=PNS, depth=16, ch=160)
    detinit.fill_module_device_(var, 16, 0, 'var.'); detinit.fill_module_device_(vae, 16, 0, 'vae.')
    return vae.eval(), var.eval()


def requests(B: int, K: int):
    labels = [[(91 * (b * 8 + k) + 7) % 1000 for k in range(K)] for b in range(B)]
    return labels, [[1.0 / K] * K for _ in range(B)], [1000 + b for b in range(B)]


def kernel_bench(B: int, l: int, V: int, iters: int, reps: int) -> dict:
    import torch
    from var_amd import hip
    g = torch.Generator(device='cuda').manual_seed(0)
    noise = torch.empty(B * l, V, device='cuda').exponential_(1, generator=g)
    idx = torch.empty(B * l, dtype=torch.int64, device='cuda')
    masked, guided = torch.empty(B * l, V, device='cuda'), torch.empty(B * l, V, device='cuda')
    tk = torch.full((B,), 900, dtype=torch.int32, device='cuda')
    tp = torch.full((B,), 0.96, dtype=torch.float64, device='cuda')
    tt = torch.full((B,), 1.5, dtype=torch.float64, device='cuda')
    out = {}
    fns = {}
    for G in (2, 3, 5):
        lg = torch.randn(G * B * l, V, device='cuda', generator=g) * 3
        coef = torch.tensor([[2.5 / (G - 1)] * (G - 1) + [1.5]] * B, dtype=torch.float32, device='cuda')
        if G == 2:
            fns['cfg_sample_rows G=2'] = (lambda lg=lg: hip.call('cfg_sample_rows_f32', lg, noise, idx, masked, B, l, V, tt, tk, tp, 900), 4)
        fns[f'mix_sample_rows G={G}'] = (lambda lg=lg, coef=coef, G=G: hip.call('mix_sample_rows_f32', lg, noise, idx, masked, None, B, l, V, G, coef, tk, tp, 900), G + 2)
        fns[f'mix_sample_rows G={G} + guided_out'] = (lambda lg=lg, coef=coef, G=G: hip.call('mix_sample_rows_f32', lg, noise, idx, masked, guided, B, l, V, G, coef, tk, tp, 900), G + 3)

    def many(fn):
        return lambda: [fn() for _ in range(reps)]
    ms = rounds_ms({k: many(f) for k, (f, _) in fns.items()}, 2, iters)
    for k, (f, rows) in fns.items():
        per = [x / reps * 1e3 for x in ms[k]]
        med = statistics.median(per)
        out[k] = dict(us_per_launch=round(med, 2), min_us=round(min(per), 2), max_us=round(max(per), 2),
                      bytes=rows * B * l * V * 4, GBps=round(rows * B * l * V * 4 / med / 1e3, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--precisions', default='f32,bf16')
    ap.add_argument('--iters', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--B', type=int, default=8)
    ap.add_argument('--scored-only', action='store_true')
    ap.add_argument('--root', default=HERE)
    ap.add_argument('--parent-root', default='')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if a.iters < 5:
        ap.error('--iters must be at least 5')
    precs = a.precisions.split(',')
    B = a.B
    res = dict(model='VAR-d16 256x256, detinit seed 0', B=B, iters=a.iters, **KW)
    if a.parent_root and not a.scored_only:
        # fresh processes, one at a time, before this process opens the GPU: parent, this, parent, this
        runs = {'parent': [], 'this': []}
        for who, root in (('parent', a.parent_root), ('this', HERE)) * 2:
            cmd = [sys.executable, os.path.abspath(__file__), '--scored-only', '--root', root, '--precisions', a.precisions, '--iters', str(a.iters), '--B', str(B)]
            env = {k: v for k, v in os.environ.items() if k != 'VARHIP_LIB'}
            runs[who].append(json.loads(subprocess.run(cmd, check=True, capture_output=True, text=True, env=env).stdout.strip().splitlines()[-1])['per_image_scored'])
        res['a_per_image_scored_in_fresh_processes'] = runs
    vae, var = build_model(a.root)
    labels1, _, seeds = requests(B, 1)
    lab1 = [x[0] for x in labels1]
    out = {}
    for prec in precs:
        var.set_hip_precision(prec)
        fns = {'per_image_scored': lambda: var.autoregressive_infer_cfg_per_image_scored(lab1, seeds, **KW)}
        if not a.scored_only:
            for K in (1, 2, 4):
                lab, w, _ = requests(B, K)
                fns[f'composed K={K}'] = lambda lab=lab, w=w: var.sample_composed(lab, w, seeds, **KW)
            fns['per_image_scored (again)'] = fns['per_image_scored']
        out[prec] = {k: summary(v) for k, v in rounds_ms(fns, 2, a.iters).items()}
        if not a.scored_only:
            ref = var.autoregressive_infer_cfg_per_image_scored(lab1, seeds, **KW)
            rec = var.sample_composed(labels1, [[1.0]] * B, seeds, **KW)
            import torch
            out[prec]['K=1 equals the per-image scored call (tokens, images)'] = bool(torch.equal(ref.tokens, rec.tokens) and torch.equal(ref.images, rec.images))
            base = out[prec]['per_image_scored']['median_ms']
            out[prec]['ratio to per_image_scored'] = {k: round(v['median_ms'] / base, 4) for k, v in out[prec].items() if isinstance(v, dict) and 'median_ms' in v}
    var.set_hip_precision('f32')
    if a.scored_only:
        res['per_image_scored'] = {p: out[p]['per_image_scored'] for p in precs}
    else:
        res['b_calls'] = out
        res['c_kernel'] = dict(B=B, l=PNS[-1] ** 2, V=var.V, top_k=900, top_p=0.96, reps=a.reps, **kernel_bench(B, PNS[-1] ** 2, var.V, a.iters, a.reps))
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    print(text if not a.scored_only else json.dumps(res))


if __name__ == '__main__':
    main()
