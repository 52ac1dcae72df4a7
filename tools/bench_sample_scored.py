#!/usr/bin/env python3
"""Timing of scored sampling on one MI355X, random-init weights (detinit seed 0), VAR-d16 256 x 256, B = 64, cfg 1.5, top-k 900, top-p 0.96,
per precision, in one process, the variants of a comparison alternating call by call (2 warm-up rounds, --iters (>= 5) timed rounds, median of
HIP-event times):
  (a) VAR.autoregressive_infer_cfg_scored against VAR.autoregressive_infer_cfg (the plain call is timed twice per round, first and last:
      the difference of its two medians and the min..max of its samples are the run-to-run spread the other differences are read against);
  (b) the scored call against the plain call + VAR.token_log_likelihood on its tokens (the second transformer pass the scored call replaces);
  (c) VAR.sample_best_of at n = --n against VAR.autoregressive_infer_cfg_per_image on the B * n candidates (in batches of B) followed by
      VAR.token_log_likelihood on their tokens: the route to the same ranking without this feature (it decodes every candidate).

    python tools/bench_sample_scored.py [--precisions f32,bf16] [--iters 5] [--B 64] [--n 4] [--out profiles/sample_scored_bench.json]
    python tools/bench_sample_scored.py --plain-only [--root OTHER_CHECKOUT]     # the plain call alone, optionally of another (built) checkout

Prints one JSON object (and writes it to --out)."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

import torch

PNS = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
KW = dict(cfg=1.5, top_k=900, top_p=0.96)


def rounds_ms(fns: dict, warmup: int, iters: int) -> dict:
    """every round runs each variant once, in the dict's order, each between its own pair of events -> {name: [ms per round]}"""
    out = {k: [] for k in fns}
    for r in range(warmup + iters):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            torch.cuda.synchronize()
            if r >= warmup:
                out[name].append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--precisions', default='f32,bf16')
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--B', type=int, default=64)
    ap.add_argument('--n', type=int, default=4)
    ap.add_argument('--plain-only', action='store_true')
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if a.iters < 5:
        ap.error('--iters must be at least 5')
    sys.path.insert(0, os.path.abspath(a.root))
    from models import build_vae_var
    from var_amd import detinit
    B, n = a.B, a.n
    with contextlib.redirect_stdout(io.StringIO()):
        vae, var = build_vae_var(device='cuda', patch_nums=PNS, depth=16, ch=160)
    detinit.fill_module_device_(var, 16, 0, 'var.'); detinit.fill_module_device_(vae, 16, 0, 'vae.')
    var.eval(); vae.eval()
    labels = torch.arange(B, device='cuda') * 97 % 1000
    seeds = [[1000 + b * n + c for c in range(n)] for b in range(B)]
    flat_seeds = [s for row in seeds for s in row]
    flat_labels = labels.repeat_interleave(n)
    med = lambda xs: round(statistics.median(xs), 3)
    res = dict(config=dict(model='d16', B=B, n=n, warmup=2, iters=a.iters, statistic='median of HIP-event times, variants alternating per round', **KW))

    def plain():
        return var.autoregressive_infer_cfg(B, labels, g_seed=0, **KW)

    for prec in a.precisions.split(','):
        var.set_hip_precision(prec)
        if a.plain_only:
            ms = rounds_ms(dict(plain=plain), 2, a.iters)['plain']
            res[prec] = dict(plain_ms=med(ms), plain_ms_all=[round(x, 3) for x in ms])
            print(f'[bench_sample_scored] {prec}: plain {med(ms):.2f} ms', flush=True)
            continue

        def plain_then_loglik():
            tok = torch.empty(B, var.L, dtype=torch.int64, device='cuda')
            var.rng.manual_seed(0)
            var.engine().sample(B, labels, var.rng, KW['cfg'], KW['top_k'], KW['top_p'], tokens_out=tok)
            return var.token_log_likelihood(tok, labels.view(B, 1), cfg=0.0, max_rows=B)

        def per_image_then_loglik():
            best = []
            for c0 in range(0, B * n, B):
                img, tok = var.autoregressive_infer_cfg_per_image(flat_labels[c0:c0 + B], flat_seeds[c0:c0 + B], return_tokens=True, **KW)
                best.append(var.token_log_likelihood(tok, flat_labels[c0:c0 + B].view(B, 1), cfg=0.0, max_rows=B).double().sum(-1))
            return torch.cat(best)

        ab = rounds_ms(dict(plain_first=plain, scored=lambda: var.autoregressive_infer_cfg_scored(B, labels, g_seed=0, **KW),
                            plain_then_loglik=plain_then_loglik, plain_last=plain), 2, a.iters)
        c = rounds_ms(dict(best_of=lambda: var.sample_best_of(labels, seeds, by='logp_cond', max_images=B, **KW),
                           per_image_then_loglik=per_image_then_loglik), 2, a.iters)
        p1, p2, sc, pl = med(ab['plain_first']), med(ab['plain_last']), med(ab['scored']), med(ab['plain_then_loglik'])
        bo, pil = med(c['best_of']), med(c['per_image_then_loglik'])
        allp = ab['plain_first'] + ab['plain_last']
        res[prec] = dict(plain_ms=med(allp), plain_first_ms=p1, plain_last_ms=p2, plain_min_ms=round(min(allp), 3), plain_max_ms=round(max(allp), 3),
                         scored_ms=sc, scored_minus_plain_ms=round(sc - med(allp), 3), plain_then_loglik_ms=pl, scored_over_plain_then_loglik=round(sc / pl, 4),
                         best_of_ms=bo, per_image_then_loglik_ms=pil, best_of_over_per_image_then_loglik=round(bo / pil, 4),
                         all={k: [round(x, 3) for x in v] for k, v in {**ab, **c}.items()})
        print(f'[bench_sample_scored] {prec}: plain {med(allp):.2f} ms (first {p1:.2f}, last {p2:.2f}, min {min(allp):.2f}, max {max(allp):.2f}), '
              f'scored {sc:.2f} ms, plain + token_log_likelihood {pl:.2f} ms; best-of-{n} {bo:.2f} ms, per-image x {n} + token_log_likelihood {pil:.2f} ms',
              flush=True)
    var.set_hip_precision('f32')
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
