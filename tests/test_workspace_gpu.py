"""What the sampling engine keeps resident, pinned buffer by buffer.

One fixed sequence of public calls on the tiny model (depth 2, C = 128, patch_nums (1, 2, 3)) under the 'auto' precision policy, in f32 and then,
inside a bf16 autocast region, the sampling and teacher-forced ones again, reaches every kind of buffer set the engine caches: the plain
sampling set, a composed pass's, the stages of sample_best_of_pruned (sample_smc shares the first), the teacher-forced set through the last
scale and the short one behind a pruning boundary of classify.  The names, shapes and dtypes of everything in the three caches, keyed without
the stream id, and the bytes of the storages behind them must equal tests/golden/workspace_layout.json, which is the record of the revision
before the four hand-written buffer lists became one spec (d967b26); so must what an explicit switch back to 'f32' leaves.  That revision
allocated a composed pass's `x`, `cond` and `cond_silu` twice; the peak of the sample_composed step above what was live before it may not
exceed its peak.

    python tests/test_workspace_gpu.py --write PATH        records the fixture with the engine of the checkout it runs in
"""
import contextlib
import io
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'workspace_layout.json')
CACHES = ('_ws', '_ws_tf', '_ws_bop')
PNS = (1, 2, 3)
KW = dict(cfg=1.5, top_k=900, top_p=0.96)


def _describe(v):
    if isinstance(v, torch.Tensor):
        return [list(v.shape), str(v.dtype)]
    if isinstance(v, (list, tuple)):
        return [_describe(x) for x in v]
    if isinstance(v, dict):
        return {str(k): _describe(x) for k, x in v.items()}
    assert v is None or isinstance(v, int), type(v)
    return v


def _tensors(v):
    if isinstance(v, torch.Tensor):
        yield v
    elif isinstance(v, (list, tuple, dict)):
        for x in (v.values() if isinstance(v, dict) else v):
            yield from _tensors(x)


def snapshot(eng) -> dict:
    """{cache: {key without the stream id: {name: (shape, dtype)}}} and the bytes of the distinct storages behind all of it"""
    layout, storages = {}, {}
    for cache in CACHES:
        sets = layout[cache] = {}
        for key, ws in getattr(eng, cache).items():
            assert isinstance(ws, dict)
            name = ' '.join(str(k) for k in key[:1] + key[2:])
            assert name not in sets
            sets[name] = {k: _describe(v) for k, v in ws.items() if k != 'dev'}
            for t in _tensors(ws):
                storages[t.untyped_storage().data_ptr()] = t.untyped_storage().nbytes()
    return dict(layout=layout, bytes=sum(storages.values()))


def run_sequence() -> dict:
    from models import build_vae_var
    from var_amd.detinit import fill_module_

    torch.cuda.set_device(0)
    with contextlib.redirect_stdout(io.StringIO()):
        vae, var = build_vae_var(device='cuda', patch_nums=PNS, depth=2, ch=32)
    fill_module_(var, 2, 0, 'var.'); fill_module_(vae, 2, 0, 'vae.')
    var.eval()
    assert (var.C, var.num_heads, var.V, var.Cvae, var.blocks[0].ffn.fc1.weight.shape[0]) == (128, 2, 4096, 32, 512)
    eng = var.engine()
    assert not any(getattr(eng, c) for c in CACHES)
    lab = torch.tensor([3, 7], device='cuda')
    gt = ((torch.arange(2 * var.L).view(2, var.L) * 37) % var.V).cuda()
    var.set_hip_precision('auto')

    def sampling():
        var.autoregressive_infer_cfg(2, lab, g_seed=0, **KW)

    def teacher_forced():
        var.token_log_likelihood(gt, [3, 7], cfg=1.5)
        var.classify(gt, [3, 7], cfg=1.5, keep={0: 1})

    sampling()
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats(); base = torch.cuda.memory_allocated()
    var.sample_composed(torch.tensor([[3, 7], [7, 9]], device='cuda'), [[0.5, 0.5], [1.0, -0.5]], [1, 2], **KW)
    torch.cuda.synchronize(); composed_peak = torch.cuda.max_memory_allocated() - base
    var.sample_best_of_pruned(lab, [[11, 12, 13, 14], [21, 22, 23, 24]], {0: 2}, n=4, **KW)
    var.sample_smc(lab, [[11, 12], [21, 22]], resample=(0,), n=2, **KW)
    teacher_forced()
    with torch.autocast('cuda', dtype=torch.bfloat16):
        sampling()
        teacher_forced()
    torch.cuda.synchronize()
    out = dict(both=snapshot(eng), composed_peak=composed_peak)
    var.set_hip_precision('f32')                            # an explicit switch away from the last call's bf16: its sets go
    out['f32_only'] = snapshot(eng)
    return out


def test_resident_buffers_equal_the_record():
    with open(FIXTURE) as fh:
        want = json.load(fh)
    got = json.loads(json.dumps(run_sequence()))
    print('composed peak', got['composed_peak'], 'recorded', want['composed_peak'], '| bytes', got['both']['bytes'], 'recorded', want['both']['bytes'])
    for state in ('both', 'f32_only'):
        assert sorted(got[state]['layout']) == sorted(CACHES)
        for cache in CACHES:
            assert sorted(got[state]['layout'][cache]) == sorted(want[state]['layout'][cache]), (state, cache)
            for key, bufs in want[state]['layout'][cache].items():
                assert got[state]['layout'][cache][key] == bufs, (state, cache, key)
        assert got[state]['bytes'] == want[state]['bytes'], state
    assert any(k.split()[1] == 'bf16' for k in got['both']['layout']['_ws']) and all(k.split()[1] == 'f32' for c in CACHES for k in got['f32_only']['layout'][c])
    assert got['composed_peak'] <= want['composed_peak']


if __name__ == '__main__':
    assert len(sys.argv) == 3 and sys.argv[1] == '--write', 'usage: test_workspace_gpu.py --write PATH'
    with open(sys.argv[2], 'w') as fh:
        json.dump(run_sequence(), fh, indent=1, sort_keys=True)
        fh.write('\n')
