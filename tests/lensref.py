"""What tests/test_logit_lens_cpu.py and the GPU tests of VAR.logit_lens share: the per-token definitions of varhip_token_lens_f32 evaluated
independently in numpy float64 (nll / pred / rank: evalref.token_defs), the planted rows, and the derived error bars ("Logit lens")."""
import numpy as np
import torch

from tests import evalref

U = 2.0 ** -24
C_BAR = 48.0           # entropy and kl: |got - ref| <= C_BAR * 2^-24 * (|ref| + max|z_layer| + max|z_final| + log V), V <= 8192
SENT_F, SENT_I = -12345.0, -777


def kernel_bar_ok(lp, lp64, z):
    """tests/test_likelihood_gpu.py's bar of the row pass: |lp - lp64| <= 1e-6 (|lp64| + max_v |z_v| + 8) per token; numpy"""
    zmax = np.abs(z).max(-1).astype(np.float64)
    err = np.abs(lp.astype(np.float64) - lp64)
    return bool((err - 1e-6 * (np.abs(lp64) + zmax + 8) <= 0).all()), float(err.max())


def lens_defs(z, zf, gt, drop_last=False):
    """z, zf (rows, V) fp32 logits of a layer and of the final block, gt (rows,) tokens in [0, V) -> nll, entropy, kl float64, pred, rank int64.
    entropy = -sum p log p (0 log 0 = 0), kl = sum pf (log pf - log p) (pf = 0 adds 0), both from float64 log-softmaxes; an element 87 or more
    below its row's maximum has probability 0, as the contract's vm_exp has it (what that drops is below V * 88 * e^-87); drop_last: the planted
    fault, the same two sums without the last element of the row"""
    z = np.asarray(z, np.float32)
    zf = np.asarray(zf, np.float32)
    nll, _, pred, rank = evalref.token_defs(z, gt)
    ent, kl = np.empty(z.shape[0]), np.empty(z.shape[0])
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for i in range(z.shape[0]):
            a, f = z[i].astype(np.float64), zf[i].astype(np.float64)
            ent[i] = kl[i] = np.nan
            if np.isnan(a).any():
                continue
            lp = (a - a.max()) - np.log(np.exp(a - a.max()).sum())
            p = np.exp(lp)
            n = z.shape[1] - (1 if drop_last else 0)
            k = (a - a.max() > -87.0)[:n]
            ent[i] = -(p[:n][k] * lp[:n][k]).sum()
            if np.isnan(f).any():
                continue
            lpf = (f - f.max()) - np.log(np.exp(f - f.max()).sum())
            pf = np.exp(lpf)
            k = (f - f.max() > -87.0)[:n]
            kl[i] = (pf[:n][k] * (lpf[:n][k] - lp[:n][k])).sum()
    return nll, ent, kl, pred, rank


def bars_ok(got, ref, z, zf):
    """entropy / kl against float64 at C_BAR -> (ok, max |diff| over the finite references, the smallest bar); NaN and inf must match"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    same = np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])
    zmax = lambda x: np.nanmax(np.abs(np.where(np.isfinite(x), x, 0.0)), -1).astype(np.float64)
    bar = C_BAR * U * (np.abs(ref[fin]) + zmax(z)[fin] + zmax(zf)[fin] + np.log(z.shape[-1]))
    err = np.abs(got[fin] - ref[fin])
    return bool(same and (err <= bar).all()), float(err.max()), float(bar.min())


def rows(V, R, l, seed):
    """R * l >= 16 rows: the planted rows of tests/test_evaluate_gpu.py::_rows as the layer's logits, final logits that differ from them, and the
    planted pairs -> z, zf (R * l, V) fp32 and gt (R, l) int64, CPU tensors"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(R * l, V, generator=g) * 6
    z[::5, :7] += 40                                        # a few peaked rows
    gt = torch.randint(0, V, (R, l), generator=g)
    f = gt.view(-1)
    z[2, 5] = z[2, V - 1] = 60.0; f[2] = V - 1              # an exact tie at the maximum, gt the higher index: pred 5, rank 1
    z[3, 9] = z[3, 700] = 60.0; f[3] = 9                    # ... gt the lower one: pred 9, rank 0
    z[4, 100] = z[4, 500] = z[4, 900] = 0.125; f[4] = 500   # gt tied with a code on either side of it, below the maximum
    z[6, 0] = 0.0; z[6, 1] = -0.0; z[6, 2:] = -3.0; f[6] = 1    # +0 == -0
    z[7, 33] = z[7, V - 2] = float('nan'); f[7] = 40        # a NaN row: pred 33, nll NaN, NaN compares false
    f[8] = -1; f[9] = V                                     # tokens outside [0, V): NaN, rank -1, never dereferenced
    zf = z * 0.5 + torch.randn(R * l, V, generator=g) * 3
    zf[11] = z[11]                                          # a layer row equal to the final row: kl = +0.0 exactly
    zf[12] = -200.0; zf[12, 17] = 30.0; zf[12, 18] = 29.0   # a final row so peaked that pf underflows to 0 off its two peaks ...
    z[12, 100:] = float('-inf')                             # ... where the layer row holds -inf: kl finite
    zf[13] = zf[12]
    z[13] = z[12]; z[13, 17] = float('-inf')                # the same with -inf under the final arg-max: kl = +inf
    zf[14, 3] = float('nan')                                # a NaN in the final row only: kl NaN, entropy the layer row's
    return z.contiguous(), zf.contiguous(), gt


KL_ZERO, KL_FINITE, KL_INF, KL_NAN, NAN_ROW, BAD_TOKENS = 11, 12, 13, 14, 7, (8, 9)


def run_host(z, zf, gt, R, l, V):
    """varhip_token_lens_host_f32 on CPU tensors -> nll, entropy, kl (R, l) fp32, pred int64, rank int32"""
    from var_amd import hip
    o = [torch.full((R, l), SENT_F), torch.full((R, l), SENT_F), torch.full((R, l), SENT_F),
         torch.full((R, l), SENT_I, dtype=torch.int64), torch.full((R, l), SENT_I, dtype=torch.int32)]
    hip.call_host('token_lens_host_f32', z, zf, gt, l, R, l, V, *o, l)
    return o
