#!/usr/bin/env python3
"""Generate tests/golden/evidence_ref.npz by running the *reference's* per-patch class heatmap, create_heatmaps_for_classes (eval_prob.py:95,
copied into inpainting.py, smoothing.py, var_analysis.py and var_size_analysis.py), on the CPU.

The routine is loaded from the reference's eval_prob.py at run time: none of its text lives here.  That script imports packages a test machine
need not have (clip, torchvision, ...); a module that cannot be imported is replaced in sys.modules by a stub whose attributes are mocks, since
the heatmap routine itself needs only torch, numpy and matplotlib.  plt.get_cmap is wrapped so that the normalised maps the routine hands to
the colormap are recorded next to the overlays it returns.

Inputs: patch_nums (1,2,3,4,5,6,8,10,13,16), K = 2 classes, seeded scores shaped like log-probabilities (uniform in [-12, 0)), a 256 x 256
image with values k/255 in [0, 1] (the routine blends its input as given: the [-1, 1] -> [0, 1] step it computes is overwritten, DESIGN.md
§27, so the '01' form is what a fixture can pin), alpha 0.5.

Recorded: scores (K, L) fp32, image_k (3, 256, 256) uint8 (the image is image_k / 255 in fp32), norm (K, 256, 256) fp32 (what the colormap was
called with), overlays (K, 256, 256, 3) uint8, meta (JSON).

usage: gen_golden_evidence.py --reference DIR   (or VAR_REFERENCE=DIR)"""
import argparse
import importlib.util
import json
import os
import sys
import types
import typing
from unittest import mock

import numpy as np
import torch

torch.Optional = typing.Optional          # shim, see tools/gen_golden.py
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, 'tests', 'golden')
PATCH_NUMS = (1, 2, 3, 4, 5, 6, 8, 10, 13, 16)
K, SIZE, ALPHA, SEED = 2, 256, 0.5, 7
SCRIPT = 'eval_prob.py'


class _Stub(types.ModuleType):
    """stands in for a module the reference's script imports and this machine lacks: any attribute is a mock"""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        m = mock.MagicMock(name=f'{self.__name__}.{name}')
        setattr(self, name, m)
        return m


def load_routine(ref: str):
    """the reference's create_heatmaps_for_classes, from its own file; -> (function, names of the stubbed modules)"""
    sys.path.insert(0, ref)
    stubbed = []
    for _ in range(64):
        spec = importlib.util.spec_from_file_location('_ref_heatmap_script', os.path.join(ref, SCRIPT))
        mod = importlib.util.module_from_spec(spec)
        try:
            spec.loader.exec_module(mod)
            return mod.create_heatmaps_for_classes, stubbed
        except ModuleNotFoundError as e:
            parts = e.name.split('.')
            for i in range(1, len(parts) + 1):
                name = '.'.join(parts[:i])
                if name not in sys.modules:
                    sys.modules[name] = _Stub(name)
                    stubbed.append(name)
    sys.exit('gen_golden_evidence: could not import the reference script')


def inputs():
    rng = np.random.default_rng(SEED)
    L = sum(p * p for p in PATCH_NUMS)
    scores = (-12.0 * rng.random((K, L))).astype(np.float32)
    c, y, x = np.meshgrid(np.arange(3), np.arange(SIZE), np.arange(SIZE), indexing='ij')
    image_k = ((3 * x + 5 * y + 85 * c) % 256).astype(np.uint8)                  # every k in 0..255, and it compresses
    return scores, image_k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('VAR_REFERENCE'))
    ap.add_argument('--out', default=os.path.join(GOLD, 'evidence_ref.npz'))
    args = ap.parse_args()
    if not args.reference or not os.path.isfile(os.path.join(args.reference, SCRIPT)):
        sys.exit('gen_golden_evidence: give the reference checkout with --reference DIR (it is not on this machine?)')
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    routine, stubbed = load_routine(os.path.abspath(args.reference))

    scores, image_k = inputs()
    image = torch.from_numpy(image_k.astype(np.float32) / np.float32(255))
    seen = []
    real_get_cmap = plt.get_cmap

    def recording_get_cmap(*a, **kw):
        cmap = real_get_cmap(*a, **kw)

        def call(x, *b, **kb):
            seen.append(np.array(x, copy=True))
            return cmap(x, *b, **kb)
        return call
    with mock.patch.object(plt, 'get_cmap', recording_get_cmap):
        overlays = routine(torch.from_numpy(scores), list(PATCH_NUMS), image, alpha=ALPHA)
    overlays = np.stack(overlays)
    norm = np.stack(seen)
    assert overlays.shape == (K, SIZE, SIZE, 3) and overlays.dtype == np.uint8
    assert norm.shape == (K, SIZE, SIZE) and norm.dtype == np.float32 and norm.min() == 0.0 and norm.max() == 1.0
    meta = dict(patch_nums=list(PATCH_NUMS), K=K, size=SIZE, alpha=ALPHA, seed=SEED, image_range='01', scales=list(range(len(PATCH_NUMS) // 2)),
                script=SCRIPT, stubbed=stubbed, torch=torch.__version__, numpy=np.__version__, matplotlib=matplotlib.__version__)
    np.savez_compressed(args.out, scores=scores, image_k=image_k, norm=norm, overlays=overlays, meta=json.dumps(meta))
    print(f'wrote {args.out}: {os.path.getsize(args.out)} bytes; stubbed {stubbed}')


if __name__ == '__main__':
    main()
