"""What tests/test_evaluate_cpu.py and tests/test_evaluate_gpu.py share: VAR.evaluate's per-token definitions evaluated independently in numpy
(float64 where a value is compared, plain fp32 comparisons where an integer is), and the checks against the reference's own logits."""
import contextlib
import io
import json

import numpy as np
import torch

BAR = 7e-4            # the bar the project holds token_log_likelihood to on the reference fixture (tests/test_likelihood_*.py)
GAP = 1.4e-3          # two logits closer than twice that bar may change order between the reference's logits and ours
_F = {}


def fixture(golden_dir):
    """tests/golden/encode_t_pn12345.npz -> (meta, gt (2, 55) int64, the reference's VAR.forward logits (2, 55, 4096) fp32)"""
    if 'f' not in _F:
        z = np.load(f'{golden_dir}/encode_t_pn12345.npz')
        meta = json.loads(str(z['meta']))
        gt = torch.from_numpy(np.concatenate([z[f'idx_s{si}'] for si in range(len(meta['patch_nums']))], 1).astype(np.int64))
        _F['f'] = (meta, gt, torch.from_numpy(z['logits']))
    return _F['f']


def fixture_model(golden_dir, device):
    """the d2 model of the fixture with its deterministic weights, in eval mode"""
    from models import build_vae_var
    from var_amd.detinit import fill_module_
    meta = fixture(golden_dir)[0]
    with contextlib.redirect_stdout(io.StringIO()):
        vae, var = build_vae_var(device=device, patch_nums=tuple(meta['patch_nums']), depth=meta['depth'], ch=meta['ch'])
    fill_module_(var, meta['depth'], 0, 'var.'); fill_module_(vae, meta['depth'], 0, 'vae.')
    var.eval(); vae.eval()
    return vae, var


def token_defs(z, gt):
    """the definitions on fp32 logits z (..., V) and tokens gt (...): numpy, one row at a time.
    -> nll float64, smooth float64 (both from a float64 evaluation), pred int64, rank int64 (both from fp32 comparisons, as defined)"""
    z = np.asarray(z, dtype=np.float32)
    gt = np.asarray(gt, dtype=np.int64)
    V = z.shape[-1]
    zr, gr = z.reshape(-1, V), gt.reshape(-1)
    nll, smooth = np.empty(gr.shape, np.float64), np.empty(gr.shape, np.float64)
    pred, rank = np.empty(gr.shape, np.int64), np.empty(gr.shape, np.int64)
    idx = np.arange(V)
    with np.errstate(invalid='ignore', over='ignore'):
        for i, (row, g) in enumerate(zip(zr, gr)):
            r64 = row.astype(np.float64)
            nan = np.isnan(row)
            if nan.any():
                pred[i] = int(np.flatnonzero(nan)[0])                          # torch.argmax: the lowest NaN index
                m = np.nan
            else:
                m = r64.max()
                pred[i] = int(np.flatnonzero(row == row.max())[0])             # the lowest index of the maximum (+0 == -0)
            nll[i] = -((r64[g] - m) - np.log(np.exp(r64 - m).sum()))
            smooth[i] = r64[g] - r64.sum() / V
            rank[i] = int(((row > row[g]) | ((row == row[g]) & (idx < g))).sum())
    return nll.reshape(gt.shape), smooth.reshape(gt.shape), pred.reshape(gt.shape), rank.reshape(gt.shape)


def check_against_reference_fixture(var, golden_dir, device):
    """the checks of the reference fixture (ISSUE test 1 / 9) on var.evaluate, whichever route `var` takes"""
    import torch.nn.functional as F
    meta, gt, ref = fixture(golden_dir)
    V, pns = ref.shape[-1], meta['patch_nums']
    nll_ref, _, pred_ref, rank_ref = token_defs(ref.numpy(), gt.numpy())
    r = var.evaluate(gt.to(device), meta['labels'])
    assert r.images == 2 and r.nll_BL.shape == (2, var.L) and r.nll_BL.dtype == torch.float32
    assert r.pred_BL.dtype == torch.int64 and r.rank_BL.dtype == torch.int32 and r.nll_S.dtype == torch.float64 and r.correct_S.dtype == torch.int64
    err = float(np.abs(r.nll_BL.double().cpu().numpy() - nll_ref).max())
    print(f'nll vs the reference logits: max |diff| {err:.3e}')
    assert err <= BAR, f'nll vs reference logits: {err:.3e}'
    assert np.array_equal(r.pred_BL.cpu().numpy(), pred_ref), 'pred differs from the reference argmax'
    zg = np.take_along_axis(ref.numpy(), gt.numpy()[..., None], -1)
    near = (np.abs(ref.numpy() - zg) <= GAP).sum(-1) - 1                          # other codes within GAP of z_gt
    drank = np.abs(r.rank_BL.cpu().numpy().astype(np.int64) - rank_ref)
    print(f'rank: max |diff| {int(drank.max())}, max allowance {int(near.max())}')
    assert (drank <= near).all(), f'rank differs by more than the near-ties allow: {int((drank - near).max())}'
    assert r.tokens_S.tolist() == [2 * pn * pn for pn in pns]
    assert r.acc_mean == 0.0 and int(r.correct_S.sum()) == 0
    want_mean, want_tail = nll_ref.mean(), nll_ref[:, -pns[-1] ** 2:].mean()
    assert abs(r.L_mean - want_mean) <= BAR and abs(r.L_tail - want_tail) <= BAR, (r.L_mean, want_mean, r.L_tail, want_tail)
    ps = r.per_scale()
    for (b, e), pn in zip(var.begin_ends, pns):
        assert abs(ps[f'L_{16 * pn}'] - nll_ref[:, b:e].mean()) <= BAR and ps[f'acc_{16 * pn}'] == 0.0
    rs = var.evaluate(gt.to(device), meta['labels'], label_smooth=0.1)
    want = float(F.cross_entropy(ref.double().view(-1, V), gt.view(-1), label_smoothing=0.1))
    print(f'smoothed loss {rs.loss!r} vs torch on the reference logits {want!r}')
    assert abs(rs.loss - want) <= BAR and rs.label_smooth == 0.1
    assert torch.equal(rs.nll_BL, r.nll_BL) and rs.loss != r.loss
    return r
