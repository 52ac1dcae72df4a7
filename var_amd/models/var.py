"""VAR transformer with the reference's module API (models/var.py:21-190, 577-653).

`autoregressive_infer_cfg` — the hot path — is a thin shell: argument handling as in the reference, then
var_amd.engine.SamplingEngine, which runs the whole loop on HIP kernels for gfx950.  There is deliberately no PyTorch
implementation of that loop in this file: on a machine without the HIP library or a GPU the call fails loudly.
`forward` (teacher forcing, autograd) is plain PyTorch for trainer.py / likelihood scripts."""
import math
from functools import partial
from typing import NamedTuple, Optional, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from .. import dist
from . import args as A
from .args import normalize_keep, normalize_resample     # noqa: F401  (names that tests and tools import from here)
from .basic_var import AdaLNBeforeHead, AdaLNSelfAttn
from .helpers import gumbel_softmax_with_rng, sample_with_top_k_top_p_     # noqa: F401  (names the notebooks import from here)
from .vqvae import VQVAE, VectorQuantizer2


def code_distance_rows(codebook: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    """(len(rows), V) fp32 direct-form L2 distances from the codes `rows` to every code: sqrt of one fma chain over the channels in channel
    order, the arithmetic of varhip_code_dist_f32 / varhip_neighbor_table_f32.  Each fma is evaluated as the float64 sum of the exact square
    and the fp32 accumulator, rounded once more to fp32 (equal to the fused result except in rare double-rounding cases)."""
    cb = codebook.float()
    a = cb[rows]
    acc = torch.zeros(a.shape[0], cb.shape[0], dtype=torch.float32, device=cb.device)
    for c in range(cb.shape[1]):
        d = (a[:, c:c + 1] - cb[:, c].unsqueeze(0)).double()
        acc = (acc.double() + d * d).float()
    return acc.sqrt()


def token_score_torch(z: torch.Tensor, gt: torch.Tensor, desc: tuple, d: Optional[torch.Tensor]) -> torch.Tensor:
    """the per-token scores of VAR.token_scores in PyTorch.  z: (K, l, V) fp32 logits of one image's K class rows, gt: (l,) tokens,
    desc: ('group_smoothed', G) | ('neighbor_max', threshold) | ('expected_distance', top_k or 0), d: (l, V) distance rows of the gt codes"""
    K, l, V = z.shape
    g = gt.view(1, l, 1).expand(K, l, 1)
    mode, par = desc
    if mode == 'neighbor_max':
        lp = torch.log_softmax(z, dim=-1)
        return lp.masked_fill(~(d <= par).unsqueeze(0), -math.inf).amax(-1)
    p = torch.softmax(z, dim=-1)
    if mode == 'expected_distance' and par == 0:
        return -(p * d.unsqueeze(0)).sum(-1)
    order = torch.sort(z, dim=-1, descending=True, stable=True).indices        # z descending, ties by ascending index
    if mode == 'expected_distance':
        top = order[..., :par]
        pk = p.gather(-1, top)
        return -(pk * d.unsqueeze(0).expand(K, l, V).gather(-1, top)).sum(-1) / pk.sum(-1)
    G = par
    ng = (V + G - 1) // G
    ps = torch.nn.functional.pad(p.gather(-1, order), (0, ng * G - V))
    sums = ps.view(K, l, ng, G).sum(-1)
    size = (V - torch.arange(ng, device=z.device) * G).clamp(max=G).to(z.dtype)
    rank = torch.empty_like(order).scatter_(-1, order, torch.arange(V, device=z.device).expand(K, l, V))
    grp = rank.gather(-1, g) // G
    return torch.log((sums / size).gather(-1, grp) + 1e-10).squeeze(-1)


class ClassifyResult(NamedTuple):
    """VAR.classify's result: pred (N,) int64 positions into the label row, total (N, K) float64, depth (N, K) int64, tokens (N, K, L) fp32"""
    pred: torch.Tensor
    total: torch.Tensor
    depth: torch.Tensor
    tokens: torch.Tensor


class BestOfResult(NamedTuple):
    """VAR.sample_best_of_pruned's result: images (B, 3, H, W) or None, winners: the SampleRecord of the B chosen candidates, totals (B, n)
    float64 each candidate's running total at its depth, depth (B, n) int64 the last scale it was sampled through, choice (B,) int64 the best
    full-depth candidate, tokens (B, n, L) int64 every candidate's drawn tokens (-1 past its depth)"""
    images: Optional[torch.Tensor]
    winners: 'SampleRecord'
    totals: torch.Tensor
    depth: torch.Tensor
    choice: torch.Tensor
    tokens: torch.Tensor


class SMCResult(NamedTuple):
    """VAR.sample_smc's result (K = len(resample) boundaries): images (B, n, 3, H, W) or None; particles: the SampleRecord of the B * n final
    particles (row b * n + c), tokens and statistics lineage-consistent; log_weights (B, n) float64, final; ancestors (B, K, n) int64: the slot
    whose state slot c carries on from each boundary; resampled (B, K) bool; ess (B, K) float64: the effective sample size each boundary saw;
    log_weights_seen (B, K, n) float64: the log-weights each boundary decided on; patch_nums"""
    images: Optional[torch.Tensor]
    particles: 'SampleRecord'
    log_weights: torch.Tensor
    ancestors: torch.Tensor
    resampled: torch.Tensor
    ess: torch.Tensor
    log_weights_seen: torch.Tensor
    patch_nums: tuple

    def best(self) -> torch.Tensor:
        """(B,) int64: each image's particle of the highest final log-weight by VAR.classify's rule (NaN below everything, ties to the lower index)"""
        lw = self.log_weights.detach().cpu().numpy()
        return torch.tensor([int(rule_order(row)[0]) for row in lw], dtype=torch.int64, device=self.log_weights.device)


class GenerativeResult(NamedTuple):
    """VAR.classify_generative's result: pred (N,) int64 positions into the label row, score (N, K) fp32 -mean|f_in - f_rec|, tokens (N, K, L)
    int64 the reconstructions' tokens (kept prefix + greedy tokens)"""
    pred: torch.Tensor
    score: torch.Tensor
    tokens: torch.Tensor


class EvalResult:
    """VAR.evaluate's result: the validation metrics of the trainer (reference trainer.py:54-84 eval_ep, :126-156 the logging block) as SUMS on
    the model's device, so that batches and ranks can be added (`a + b`, or an all-reduce of the stacked sums) before anything is divided.
      images       int: N
      nll_S        (S,) float64: per scale the sum over images and tokens of -log p(gt)
      smooth_S     (S,) float64: per scale the sum of z_gt - mean_v z_v; CrossEntropyLoss(label_smoothing=e) of a token is nll + e * (z_gt - mean_v z_v)
      correct_S    (S,) int64: per scale the count of pred == gt;   tokens_S (S,) int64: N * pn^2
      pred_hist_V  (V,) int64: the histogram of pred over all tokens
      nll_BL, pred_BL, rank_BL  (N, L) fp32 / int64 / int32: the per-token values; rank = the number of codes ahead of gt in the order z
                   descending, ties by ascending index (rank < k: gt is in the top k)
      label_smooth float, as passed;  patch_nums: the scales the result covers (resos: the trainer's names of them, 16 * pn)
    The derived values are plain Python floats computed in float64 from one device-to-host transfer of the sums."""
    __slots__ = ('images', 'nll_S', 'smooth_S', 'correct_S', 'tokens_S', 'pred_hist_V', 'nll_BL', 'pred_BL', 'rank_BL', 'label_smooth', 'patch_nums', '_h')

    def __init__(self, images, nll_S, smooth_S, correct_S, tokens_S, pred_hist_V, nll_BL, pred_BL, rank_BL, label_smooth, patch_nums):
        self.images, self.nll_S, self.smooth_S, self.correct_S, self.tokens_S = int(images), nll_S, smooth_S, correct_S, tokens_S
        self.pred_hist_V, self.nll_BL, self.pred_BL, self.rank_BL = pred_hist_V, nll_BL, pred_BL, rank_BL
        self.label_smooth, self.patch_nums = float(label_smooth), tuple(patch_nums)
        self._h = None

    @property
    def resos(self) -> tuple:
        return tuple(16 * pn for pn in self.patch_nums)

    def _host(self):
        """(nll_S, smooth_S, correct_S, tokens_S, pred_hist_V) as float64 numpy arrays (counts below 2^53 are exact), one transfer"""
        if self._h is None:
            S = self.nll_S.shape[0]
            flat = torch.cat((self.nll_S, self.smooth_S, self.correct_S.double(), self.tokens_S.double(), self.pred_hist_V.double())).cpu().numpy()
            self._h = (flat[:S], flat[S:2 * S], flat[2 * S:3 * S], flat[3 * S:4 * S], flat[4 * S:])
        return self._h

    @property
    def L_mean(self) -> float:
        """trainer.py:72: the mean cross entropy over every token"""
        nll, _, _, tok, _ = self._host()
        return float(nll.sum() / tok.sum())

    @property
    def L_tail(self) -> float:
        """trainer.py:73: the mean cross entropy over the last scale"""
        nll, _, _, tok, _ = self._host()
        return float(nll[-1] / tok[-1])

    @property
    def acc_mean(self) -> float:
        """trainer.py:74: percent of tokens with argmax == gt"""
        _, _, cor, tok, _ = self._host()
        return float(100.0 * cor.sum() / tok.sum())

    @property
    def acc_tail(self) -> float:
        """trainer.py:75: the same over the last scale"""
        _, _, cor, tok, _ = self._host()
        return float(100.0 * cor[-1] / tok[-1])

    @property
    def loss(self) -> float:
        """trainer.py:112-120 without progressive training: CrossEntropyLoss(label_smoothing) per token, weighted 1 / L, summed per image,
        averaged over the images = the mean over every token of nll + label_smooth * (z_gt - mean_v z_v)"""
        nll, smo, _, tok, _ = self._host()
        return float((nll.sum() + self.label_smooth * smo.sum()) / tok.sum())

    def per_scale(self) -> dict:
        """trainer.py:149-155: {'acc_<reso>': percent, 'L_<reso>': mean cross entropy} per scale"""
        nll, _, cor, tok, _ = self._host()
        kw = {}
        for si, reso in enumerate(self.resos):
            kw[f'acc_{reso}'] = float(100.0 * cor[si] / tok[si])
            kw[f'L_{reso}'] = float(nll[si] / tok[si])
        return kw

    @property
    def z_voc_usage(self) -> float:
        """trainer.py:140-143: percent of the codes predicted more often than 0.001 / V of the time"""
        hist = self._host()[4]
        return float(((hist / hist.sum()) > 0.001 / hist.shape[0]).mean() * 100.0)

    def topk_correct_S(self, k: int) -> torch.Tensor:
        """(S,) int64: per scale the number of tokens whose gt is among the k best codes (rank < k; k = 1: correct_S on NaN-free rows)"""
        if isinstance(k, bool) or int(k) != k or k < 1:
            raise ValueError('k must be an integer >= 1')
        hit = (self.rank_BL >= 0) & (self.rank_BL < int(k))
        ends = np.cumsum([pn * pn for pn in self.patch_nums]).tolist()
        return torch.stack([hit[:, e - pn * pn:e].sum() for e, pn in zip(ends, self.patch_nums)]).to(torch.int64)

    def __add__(self, other):
        if not isinstance(other, EvalResult):
            return NotImplemented
        if (self.nll_S.shape != other.nll_S.shape or self.pred_hist_V.shape != other.pred_hist_V.shape or self.label_smooth != other.label_smooth
                or self.patch_nums != other.patch_nums or self.nll_S.device != other.nll_S.device):
            raise ValueError('EvalResult +: the two results differ in their scales, vocabulary, label_smooth or device')
        return EvalResult(self.images + other.images, self.nll_S + other.nll_S, self.smooth_S + other.smooth_S, self.correct_S + other.correct_S,
                          self.tokens_S + other.tokens_S, self.pred_hist_V + other.pred_hist_V, torch.cat((self.nll_BL, other.nll_BL)),
                          torch.cat((self.pred_BL, other.pred_BL)), torch.cat((self.rank_BL, other.rank_BL)), self.label_smooth, self.patch_nums)

    def __repr__(self):
        return (f'EvalResult(images={self.images}, L_mean={self.L_mean:.4f}, L_tail={self.L_tail:.4f}, acc_mean={self.acc_mean:.2f}, '
                f'acc_tail={self.acc_tail:.2f}, label_smooth={self.label_smooth})')


def token_eval_torch(z: torch.Tensor, gt: torch.Tensor):
    """VAR.evaluate's per-token definitions in PyTorch.  z: (n, l, V) fp32 logits, gt: (n, l) tokens -> (nll fp32, smooth fp32, pred int64, rank int32)"""
    V = z.shape[-1]
    g = gt.unsqueeze(-1)
    nll = -torch.log_softmax(z, dim=-1).gather(-1, g).squeeze(-1)
    zg = z.gather(-1, g)
    ahead = (z > zg) | ((z == zg) & (torch.arange(V, device=z.device) < g))
    smooth = (zg.squeeze(-1).double() - z.double().sum(-1) / V).float()
    return nll, smooth, z.argmax(-1), ahead.sum(-1).to(torch.int32)


MASS_ONE = float(2 ** 48)            # the fixed point of the probability mass: q_v = rint(p_v * 2^48)


class DistanceProfile:
    """VAR.distance_profile's result: per image n, candidate class k, scale s and distance bin b (edges[b] <= d < edges[b + 1]) the codes v of
    every token's row with d(gt, v) in the bin and p_v > min_prob, on the model's device:
      count_NKSB   (N, K, S, B) int64: how many (token, code) pairs fall in the bin
      mass_q_NKSB  (N, K, S, B) int64: the sum of their q_v = rint(p_v * 2^48), p_v the fp32 softmax probability: integer sums, the same bits
                   whatever the packing, the class order or the run; a cell is at most pn_s^2 * 2^48 <= 2^58
      mass_NKSB    (N, K, S, B) float64: mass_q * 2^-48, the probability mass in the bin
      edges (B + 1,) fp32, min_prob float (the fp32 value used), patch_nums: the scales the result covers
    mean_prob() is the curve the fork plots (var_analysis.py:694-732, :798-818): the mean probability of the pairs of a bin."""
    __slots__ = ('count_NKSB', 'mass_q_NKSB', 'edges', 'min_prob', 'patch_nums')

    def __init__(self, count_NKSB, mass_q_NKSB, edges, min_prob, patch_nums):
        self.count_NKSB, self.mass_q_NKSB, self.edges = count_NKSB, mass_q_NKSB, edges
        self.min_prob, self.patch_nums = float(min_prob), tuple(patch_nums)

    @property
    def mass_NKSB(self) -> torch.Tensor:
        return self.mass_q_NKSB.double() / MASS_ONE

    def mean_prob(self, over_images: bool = False) -> torch.Tensor:
        """mass / count in float64, NaN where count == 0: (N, K, S, B), or (K, S, B) with over_images=True (both summed over N first)"""
        mass, count = self.mass_NKSB, self.count_NKSB.double()
        if over_images:
            mass, count = mass.sum(0), count.sum(0)
        return torch.where(count > 0, mass / count, torch.full_like(mass, math.nan))

    def centers(self) -> torch.Tensor:
        """(B,) float64 bin centres (edges[b] + edges[b + 1]) / 2 (inf for a last bin that reaches +inf)"""
        e = self.edges.double()
        return (e[:-1] + e[1:]) / 2

    def __repr__(self):
        N, K, S, B = self.count_NKSB.shape
        return f'DistanceProfile(images={N}, classes={K}, scales={S}, bins={B}, min_prob={self.min_prob})'


def distance_profile_torch(z: torch.Tensor, gt: torch.Tensor, dist: torch.Tensor, edges: torch.Tensor, min_prob: float):
    """VAR.distance_profile's definitions in PyTorch for one scale of one image.  z: (K, l, V) fp32 logits of the image's K class rows, gt:
    (l,) tokens, dist: (l, V) fp32 distance rows of the gt codes, edges: (B + 1,) fp32 ascending, min_prob: an fp32 value
    -> (count (K, B) int64, mass_q (K, B) int64).  p = softmax(z) in fp32; a pair is in bin b iff edges[b] <= d < edges[b + 1] and
    p > min_prob (a NaN is in no bin); a token outside [0, V) contributes nothing."""
    K, l, V = z.shape
    B = edges.numel() - 1
    edges = edges.to(z.device, torch.float32)
    p = torch.softmax(z.float(), dim=-1)
    d = dist.to(torch.float32).unsqueeze(0).expand(K, l, V).contiguous()
    b = torch.bucketize(d, edges, right=True) - 1                       # |{i : edges[i] <= d}| - 1
    ok = (b >= 0) & (b < B) & ~torch.isnan(d) & (p > torch.tensor(min_prob, dtype=torch.float32, device=z.device))
    ok = ok & ((gt >= 0) & (gt < V)).view(1, l, 1)
    q = torch.where(ok, torch.round(p.double() * MASS_ONE), torch.zeros((), dtype=torch.float64, device=z.device)).to(torch.int64)
    cell = (torch.arange(K, device=z.device).view(K, 1, 1) * B + b.clamp(0, B - 1))[ok]
    count = torch.zeros(K * B, dtype=torch.int64, device=z.device).index_add_(0, cell, torch.ones_like(cell))
    mass = torch.zeros(K * B, dtype=torch.int64, device=z.device).index_add_(0, cell, q[ok])
    return count.view(K, B), mass.view(K, B)


H_ONE = float(2 ** 40)               # the fixed point of sum_k pi_k H_k: rint(pi_k * H_k * 2^40)
CLASS_INFO_MAX_CAND = 16384          # candidates per image of VAR.class_information (the cap of classify)


class ClassInformation:
    """VAR.class_information's result: per token, how much the class changes the model's prediction, on the model's device (nats):
      entropy   (N, K, L) fp32: H(p_k), p_k the softmax of the (guided) logits of class k
      h_mix     (N, L) fp32: H(sum_k pi_k p_k), the entropy of the mixture over the classes
      h_cond    (N, L) fp32: sum_k pi_k H(p_k)
      mi        (N, L) fp32: h_mix - h_cond from the unrounded operands: I(c ; x_t | x_<t), between 0 and H(pi) up to rounding
      logp_mix  (N, L) fp32: log sum_k pi_k p_k(gt), the model-averaged likelihood of the ground-truth token
      prior     (N, K) fp32 as used, patch_nums: the scales the result covers
    The sums over classes are integer sums in fixed point (2^-48 for the mixture, 2^-40 for h_cond): the (N, L) fields are bit-equal across
    max_rows, packing, class order and repeated calls."""
    __slots__ = ('entropy', 'h_mix', 'h_cond', 'mi', 'logp_mix', 'prior', 'patch_nums')

    def __init__(self, entropy, h_mix, h_cond, mi, logp_mix, prior, patch_nums):
        self.entropy, self.h_mix, self.h_cond, self.mi, self.logp_mix, self.prior = entropy, h_mix, h_cond, mi, logp_mix, prior
        self.patch_nums = tuple(patch_nums)

    def per_scale(self) -> dict:
        """{'mi_sum', 'mi_mean', 'h_mix_sum', 'h_mix_mean', 'h_cond_sum', 'h_cond_mean'}: (N, S) float64 each, per image and scale the sum and
        the mean over the scale's tokens"""
        out = {}
        for name in ('mi', 'h_mix', 'h_cond'):
            x, cur, sums = getattr(self, name).double(), 0, []
            for pn in self.patch_nums:
                sums.append(x[:, cur:cur + pn * pn].sum(-1))
                cur += pn * pn
            out[name + '_sum'] = torch.stack(sums, -1)
            out[name + '_mean'] = out[name + '_sum'] / torch.tensor([pn * pn for pn in self.patch_nums], dtype=torch.float64, device=x.device)
        return out

    def mi_map(self, **kw) -> 'EvidenceMaps':
        """evidence_maps(mi[:, None, :], patch_nums, **kw): where in the image the class information sits (one 'class': the map of mi)"""
        return evidence_maps(self.mi[:, None, :].contiguous(), self.patch_nums, **kw)

    def __repr__(self):
        N, K, L = self.entropy.shape
        return f'ClassInformation(images={N}, classes={K}, tokens={L}, scales={len(self.patch_nums)})'


def class_information_torch(z: torch.Tensor, gt: torch.Tensor, prior: torch.Tensor, max_rows: Optional[int] = None):
    """VAR.class_information's definitions in PyTorch for one scale of one image.  z: (K, l, V) fp32 logits of the image's K class rows (the
    guided combination when cfg > 0), gt: (l,) tokens, prior: (K,) fp32 -> (entropy (K, l), h_mix, h_cond, mi, logp_mix (l,)) fp32.
    p_k = softmax(z_k) evaluated in float64 and rounded once to fp32, H_k likewise; the sums over classes are the fixed-point integer sums of
    include/var_hip.h (rint(p pi 2^48), rint(pi H 2^40)), added max_rows class rows at a time (None: all at once): the result does not depend
    on max_rows.  A NaN in any class row of a token makes its four per-token values NaN; a token outside [0, V): logp_mix NaN."""
    K, l, V = z.shape
    dev = z.device
    pi = prior.to(dev, torch.float32).double()
    step = K if max_rows is None else max(1, int(max_rows))
    mix_q = torch.zeros(l, V, dtype=torch.int64, device=dev)
    hq = torch.zeros(l, dtype=torch.int64, device=dev)
    bad = torch.zeros(l, dtype=torch.bool, device=dev)
    ent = torch.empty(K, l, dtype=torch.float32, device=dev)
    for k0 in range(0, K, step):
        zz = z[k0:k0 + step].double()
        nanrow = torch.isnan(zz).any(-1)                                    # (k, l)
        lp = torch.log_softmax(zz, dim=-1)
        p = lp.exp()
        H = (-(torch.where(p > 0, p * lp, torch.zeros_like(p))).sum(-1)).float()
        H = torch.where(nanrow, torch.full_like(H, math.nan), H)
        ent[k0:k0 + step] = H
        pk = pi[k0:k0 + step]
        q = torch.round(p.float().double() * pk.view(-1, 1, 1) * MASS_ONE)
        q = torch.where(nanrow.unsqueeze(-1) | torch.isnan(q), torch.zeros_like(q), q)
        mix_q += q.to(torch.int64).sum(0)
        hq += torch.where(nanrow, torch.zeros_like(H, dtype=torch.float64), torch.round(pk.view(-1, 1) * H.double() * H_ONE)).to(torch.int64).sum(0)
        bad |= nanrow.any(0)
    qv = (mix_q.double() / MASS_ONE).float()
    a = torch.where(qv > 0, qv.double() * torch.log(qv).double(), torch.zeros_like(qv, dtype=torch.float64)).sum(-1)
    hc = hq.double() / H_ONE
    nan = torch.full((l,), math.nan, dtype=torch.float32, device=dev)
    valid = (gt >= 0) & (gt < V)
    qg = qv.gather(-1, torch.where(valid, gt, torch.zeros_like(gt)).view(l, 1)).squeeze(-1)
    h_mix = torch.where(bad, nan, (0.0 - a).float())
    h_cond = torch.where(bad, nan, hc.float())
    mi = torch.where(bad, nan, ((0.0 - a) - hc).float())
    logp = torch.where(bad | ~valid, nan, torch.log(qg))
    return ent, h_mix, h_cond, mi, logp


SHARE_ONE = 2 ** 21                  # the fixed point of an attention share: floor(W_bin * 2^21 / Z)
ATTN_W_ONE = float(2 ** 30)          # ... and of a softmax numerator: rint(exp(s - max s) * 2^30)


class AttentionProfile:
    """VAR.attention_profile's result: where the attention of every selected block goes, by scale, on the model's device.
      share_q      (N, D', H, S, S + 1) int64 [n, d, h, sq, b]: the sum over the pn[sq]^2 queries of scale sq of each query's fixed-point share
                   (units of 2^-21 = 1 / SHARE_ONE, truncated) on bin b.  Bins 0 .. S-1: the key's scale (0 above sq: block-causal); bin S, "near":
                   the keys of the query's own scale whose grid position is within Chebyshev distance `radius` of the query's, itself included
      nan_queries  (N, D', H, S) int32: queries with a NaN score (or no finite maximum); they add nothing to share_q
      tokens       None, or (N, D', H, L, S + 1) int32 with return_tokens=True: every query's own shares, -1 in every entry of a NaN query
      layers (the D' block indices), radius, patch_nums
    Integer sums of integer shares: the same bits whatever the packing (max_rows), the batch neighbours or the call history."""
    __slots__ = ('share_q', 'nan_queries', 'tokens', 'patch_nums', 'radius', 'layers')

    def __init__(self, share_q, nan_queries, tokens, patch_nums, radius, layers):
        self.share_q, self.nan_queries, self.tokens = share_q, nan_queries, tokens
        self.patch_nums, self.radius, self.layers = tuple(patch_nums), int(radius), tuple(layers)

    def _per_unit(self, x: torch.Tensor) -> torch.Tensor:
        """x (N, D', H, S, ...) int64 sums over a scale's queries -> float64 means over the queries that counted (NaN where none did)"""
        n = torch.tensor([pn * pn for pn in self.patch_nums], dtype=torch.float64, device=x.device) - self.nan_queries.double()
        n = n.view(*n.shape, *([1] * (x.dim() - n.dim())))
        return x.double() / (SHARE_ONE * n)

    def scale_matrix(self) -> torch.Tensor:
        """(N, D', H, S, S) float64 [.., sq, sk]: the mean share of a query of scale sq on the keys of scale sk; a row sums to 1 up to the
        truncation (at most S / SHARE_ONE below)"""
        return self._per_unit(self.share_q[..., :-1])

    def near(self) -> torch.Tensor:
        """(N, D', H, S) float64: the mean share on the query's own neighbourhood (radius)"""
        return self._per_unit(self.share_q[..., -1])

    def own_scale(self) -> torch.Tensor:
        """(N, D', H, S) float64: the mean share on the query's own scale, the diagonal of scale_matrix()"""
        return self._per_unit(torch.diagonal(self.share_q[..., :-1], dim1=-2, dim2=-1))

    def per_layer(self) -> dict:
        """{'scale_matrix': (N, D', S, S), 'near': (N, D', S), 'own_scale': (N, D', S)} float64: the means over the heads"""
        return dict(scale_matrix=self.scale_matrix().mean(2), near=self.near().mean(2), own_scale=self.own_scale().mean(2))

    def __repr__(self):
        N, D, H, S = self.nan_queries.shape
        return f'AttentionProfile(images={N}, layers={D}, heads={H}, scales={S}, radius={self.radius})'


def attention_profile_torch(var, gt: torch.Tensor, label: torch.Tensor, radius: int, layers: tuple, return_tokens: bool = False):
    """VAR.attention_profile's definitions in PyTorch on the module stack (CPU models, non-HIP tensors; the arithmetic follows the parameters' dtype).
    gt (N, L) tokens, label (N,) labels, layers: block indices, ascending -> (share_q, nan_queries, tokens or None) as in AttentionProfile.
    Per block the modules produce q and k (SelfAttention._heads, then the l2 norm and temperature, or `scale`); the scores take the block-causal
    mask, and from there float64: w = rint(exp(s - max s) * 2^30), integer sums per key scale and over the near keys, share = floor(W * 2^21 / Z),
    integer sums over a scale's queries (include/var_hip.h, varhip_attn_profile_f32: the same quantisation, fed by PyTorch's q and k).  One image
    at a time, so an image's integers do not depend on its batch neighbours."""
    dev = gt.device
    N, L, S, H = gt.shape[0], var.L, len(var.patch_nums), var.num_heads
    dt = var.pos_start.dtype
    mask = var.attn_bias_for_masking[:, :, :L, :L].to(dt)
    scale_of = var.lvl_1L[0, :L].to(dev)                                                       # (L,) the scale of every position
    seg = torch.nn.functional.one_hot(scale_of, S).double()                                    # (L, S) key -> its scale bin
    pn_of = torch.tensor([pn for pn in var.patch_nums for _ in range(pn * pn)], device=dev)
    pos = torch.cat([torch.arange(pn * pn, device=dev) for pn in var.patch_nums])
    py, px = pos // pn_of, pos % pn_of
    near = ((scale_of[:, None] == scale_of[None, :]) & ((py[:, None] - py[None, :]).abs() <= radius) & ((px[:, None] - px[None, :]).abs() <= radius)).double()
    slot = {bi: d for d, bi in enumerate(layers)}
    share = torch.zeros(N, len(layers), H, S, S + 1, dtype=torch.int64, device=dev)
    nanq = torch.zeros(N, len(layers), H, S, dtype=torch.int32, device=dev)
    tokens = torch.zeros(N, len(layers), H, L, S + 1, dtype=torch.int32, device=dev) if return_tokens else None
    for n in range(N):
        cond = var.class_emb(label[n:n + 1])
        sos = cond.unsqueeze(1).expand(1, var.first_l, -1) + var.pos_start.expand(1, var.first_l, -1)
        x_in = var.vae_proxy[0].quantize.idxBl_to_var_input([gt[n:n + 1, b:e] for b, e in var.begin_ends])
        x = torch.cat((sos, var.word_embed(x_in.to(dt))), dim=1) if L > var.first_l else sos
        x = x + var.lvl_embed(var.lvl_1L[:, :L].expand(1, -1)) + var.pos_1LC[:, :L]
        cond_or_gss = var.shared_ada_lin(cond)
        for bi, blk in enumerate(var.blocks):
            d = slot.get(bi)
            if d is not None:
                at = blk.attn
                _, _, scale1, _, shift1, _ = blk._six(cond_or_gss)
                q, k, _ = at._heads(blk.ln_wo_grad(x) * (scale1 + 1) + shift1)
                if at.attn_l2_norm:
                    q = torch.nn.functional.normalize(q, dim=-1) * at.scale_mul_1H11.clamp_max(at.max_scale_mul).exp()
                    k = torch.nn.functional.normalize(k, dim=-1)
                sc = (q @ k.transpose(-1, -2)) * at.scale + mask                                 # (1, H, L, L) in the modules' dtype
                sc = sc[0].double()
                bad = torch.isnan(sc).any(-1) | ~torch.isfinite(sc.max(-1).values)               # (H, L)
                w = torch.round(torch.exp(sc - sc.max(-1, keepdim=True).values) * ATTN_W_ONE)
                w = torch.where(torch.isnan(w), torch.zeros_like(w), w)                          # float64 integers <= 2^30: sums below 2^53 are exact
                Wb = torch.cat((w @ seg, (w * near).sum(-1, keepdim=True)), -1).to(torch.int64)  # (H, L, S + 1)
                Z = Wb[..., :S].sum(-1, keepdim=True).clamp_min(1)
                tok = torch.div(Wb << 21, Z, rounding_mode='floor')
                good = (~bad).to(torch.int64)
                share[n, d].index_add_(1, scale_of, tok * good.unsqueeze(-1))                    # integer sums over the queries of a scale
                nanq[n, d].index_add_(1, scale_of, bad.to(torch.int32))
                if return_tokens:
                    tokens[n, d] = torch.where(bad.unsqueeze(-1), torch.full_like(tok, -1), tok).to(torch.int32)
            x = blk(x=x, cond_BD=cond_or_gss, attn_bias=mask)
    return share, nanq, tokens


class _TokenMaps:
    """what AttentionMaps and AttentionRollout share: a field (..., T, L) of per-target weights over the L key positions"""
    __slots__ = ()
    _FIELD = ''

    def _begins(self) -> list:
        b = [0]
        for pn in self.patch_nums:
            b.append(b[-1] + pn * pn)
        return b

    def scale_mass(self) -> torch.Tensor:
        """(..., T, S) float64: every target's weight on the keys of each scale (0 above the target's own scale: block-causal)"""
        x, b = getattr(self, self._FIELD).double(), self._begins()
        return torch.stack([x[..., b0:b1].sum(-1) for b0, b1 in zip(b, b[1:])], -1)

    def scale_maps(self, si: int) -> torch.Tensor:
        """(..., T, pn, pn): every target's weights on the grid of scale si, a view of the field"""
        si = A.integer(si, f'si must be a scale index in [0, {len(self.patch_nums)})', 0, len(self.patch_nums) - 1)
        x, b, pn = getattr(self, self._FIELD), self._begins(), self.patch_nums[si]
        return x[..., b[si]:b[si + 1]].unflatten(-1, (pn, pn))


class AttentionMaps(_TokenMaps):
    """VAR.attention_maps' result: which positions the target tokens read, per selected block and head, on the model's device.
      rows         (N, D', H, T, L) fp32 [n, d, h, s, j]: softmax_j(q_t . k_j) of target s = token t over the keys it sees (those of its own and
                   of the coarser scales), exactly +0 at the others: a row sums to 1
      nan_queries  (N, D', H) int32: queries (of all L, targets or not) with a NaN score or no finite maximum; a target among them has a NaN row
      targets (the T flat token indices), layers (the D' block indices), patch_nums
    A row depends on its own image, block, head and target only: the same bits whatever max_rows, the batch neighbours, the other targets,
    the other selected layers or the call history."""
    __slots__ = ('rows', 'nan_queries', 'targets', 'layers', 'patch_nums')
    _FIELD = 'rows'

    def __init__(self, rows, nan_queries, targets, layers, patch_nums):
        self.rows, self.nan_queries = rows, nan_queries
        self.targets, self.layers, self.patch_nums = tuple(targets), tuple(layers), tuple(patch_nums)

    def __repr__(self):
        N, D, H, T, L = self.rows.shape
        return f'AttentionMaps(images={N}, layers={D}, heads={H}, targets={T}, tokens={L})'


class AttentionRollout(_TokenMaps):
    """VAR.attention_rollout's result: where the target tokens' information comes from through all selected blocks (Abnar & Zuidema).
      flow         (N, T, L) fp32 [n, s, j]: target s's one-hot row pushed through the selected layers from last to first,
                   r <- (1 - alpha) r + alpha r Pbar_l, Pbar_l the head mean of softmax(QK^T) under the block-causal mask: non-negative, sums to 1
      nan_queries  (N, D', H) int32 as in AttentionMaps; a NaN query that a target reaches makes that target's flow NaN at the keys it sees
      targets, layers, alpha, patch_nums
    flow is in evidence_maps' (N, K, L) score layout: evidence(**kw) draws it."""
    __slots__ = ('flow', 'nan_queries', 'targets', 'layers', 'alpha', 'patch_nums')
    _FIELD = 'flow'

    def __init__(self, flow, nan_queries, targets, layers, alpha, patch_nums):
        self.flow, self.nan_queries, self.alpha = flow, nan_queries, float(alpha)
        self.targets, self.layers, self.patch_nums = tuple(targets), tuple(layers), tuple(patch_nums)

    def evidence(self, **kw) -> 'EvidenceMaps':
        """evidence_maps(flow, patch_nums, **kw): the rollout of every target over the image (one 'class' per target)"""
        return evidence_maps(self.flow.contiguous(), self.patch_nums, **kw)

    def __repr__(self):
        N, T, L = self.flow.shape
        return f'AttentionRollout(images={N}, layers={len(self.layers)}, targets={T}, tokens={L}, alpha={self.alpha:g})'


def _attention_probs_torch(var, gt: torch.Tensor, label: torch.Tensor, layers: tuple):
    """yields (n, d, P (H, L, L) float64, bad (H, L) bool) per image n and selected block layers[d], ascending: the dense block-causal
    softmax(QK^T) of the module stack (q and k as in attention_profile_torch, in the parameters' dtype; from the scores on float64)"""
    L = var.L
    dt = var.pos_start.dtype
    mask = var.attn_bias_for_masking[:, :, :L, :L].to(dt)
    slot = {bi: d for d, bi in enumerate(layers)}
    for n in range(gt.shape[0]):
        cond = var.class_emb(label[n:n + 1])
        sos = cond.unsqueeze(1).expand(1, var.first_l, -1) + var.pos_start.expand(1, var.first_l, -1)
        x_in = var.vae_proxy[0].quantize.idxBl_to_var_input([gt[n:n + 1, b:e] for b, e in var.begin_ends])
        x = torch.cat((sos, var.word_embed(x_in.to(dt))), dim=1) if L > var.first_l else sos
        x = x + var.lvl_embed(var.lvl_1L[:, :L].expand(1, -1)) + var.pos_1LC[:, :L]
        cond_or_gss = var.shared_ada_lin(cond)
        for bi, blk in enumerate(var.blocks):
            d = slot.get(bi)
            if d is not None:
                at = blk.attn
                _, _, scale1, _, shift1, _ = blk._six(cond_or_gss)
                q, k, _ = at._heads(blk.ln_wo_grad(x) * (scale1 + 1) + shift1)
                if at.attn_l2_norm:
                    q = torch.nn.functional.normalize(q, dim=-1) * at.scale_mul_1H11.clamp_max(at.max_scale_mul).exp()
                    k = torch.nn.functional.normalize(k, dim=-1)
                sc = ((q @ k.transpose(-1, -2)) * at.scale + mask)[0].double()                   # (H, L, L)
                bad = torch.isnan(sc).any(-1) | ~torch.isfinite(sc.max(-1).values)
                e = torch.exp(sc - sc.max(-1, keepdim=True).values)
                yield n, d, e / e.sum(-1, keepdim=True), bad
            x = blk(x=x, cond_BD=cond_or_gss, attn_bias=mask)


def attention_maps_torch(var, gt: torch.Tensor, label: torch.Tensor, targets: tuple, layers: tuple):
    """VAR.attention_maps' definition in PyTorch on the module stack (CPU models, non-HIP tensors): per image the dense masked softmax in float64,
    its target rows -> (rows (N, D', H, T, L) fp32, nan_queries (N, D', H) int32)"""
    dev = gt.device
    N, H = gt.shape[0], var.num_heads
    tg = torch.tensor(targets, dtype=torch.int64, device=dev)
    rows = torch.zeros(N, len(layers), H, len(targets), var.L, dtype=torch.float32, device=dev)
    nanq = torch.zeros(N, len(layers), H, dtype=torch.int32, device=dev)
    for n, d, P, bad in _attention_probs_torch(var, gt, label, layers):
        rows[n, d] = P[:, tg].float()
        nanq[n, d] = bad.sum(-1).to(torch.int32)
    return rows, nanq


def attention_rollout_torch(var, gt: torch.Tensor, label: torch.Tensor, targets: tuple, layers: tuple, alpha: float):
    """VAR.attention_rollout's definition in PyTorch on the module stack: per image the head mean of the dense masked softmax of every selected
    block in float64, and the recurrence r <- (1 - alpha) r + alpha r Pbar from the last selected block to the first, from one-hot rows
    -> (flow (N, T, L) fp32, nan_queries (N, D', H) int32)"""
    dev = gt.device
    N, H, L = gt.shape[0], var.num_heads, var.L
    tg = torch.tensor(targets, dtype=torch.int64, device=dev)
    flow = torch.zeros(N, len(targets), L, dtype=torch.float32, device=dev)
    nanq = torch.zeros(N, len(layers), H, dtype=torch.int32, device=dev)
    pbar = {}
    for n, d, P, bad in _attention_probs_torch(var, gt, label, layers):
        pbar[d] = P.mean(0)
        nanq[n, d] = bad.sum(-1).to(torch.int32)
        if d == len(layers) - 1:
            r = torch.nn.functional.one_hot(tg, L).double()
            for dd in reversed(range(len(layers))):
                r = (1.0 - alpha) * r + alpha * (r @ pbar[dd])
            flow[n] = r.float()
            pbar = {}
    return flow, nanq


class LogitLens:
    """VAR.logit_lens's result: the prediction the trained head makes from the residual stream behind every selected block, per token, on the
    model's device.  With z the head's fp32 logits behind block layers[d], p their softmax, and pf the softmax of the final logits:
      nll      (N, D', L) fp32   -log p[gt]                       (behind the model's last block: VAR.evaluate's nll_BL)
      entropy  (N, D', L) fp32   -sum_v p_v log p_v, in nats
      kl       (N, D', L) fp32   KL(pf || p) = sum_v pf_v (log pf_v - log p_v); exactly 0 behind the model's last block
      pred     (N, D', L) int64  argmax z;  rank (N, D', L) int32: |{v : z_v > z_gt or (z_v == z_gt and v < gt)}|
      layers (the D' block indices), patch_nums: the scales the result covers
    The methods run in PyTorch with float64 sums."""
    __slots__ = ('layers', 'nll', 'entropy', 'kl', 'pred', 'rank', 'patch_nums')

    def __init__(self, layers, nll, entropy, kl, pred, rank, patch_nums):
        self.layers, self.patch_nums = tuple(layers), tuple(patch_nums)
        self.nll, self.entropy, self.kl, self.pred, self.rank = nll, entropy, kl, pred, rank

    def _scale_mean(self, x: torch.Tensor) -> torch.Tensor:
        """x (N, D', L) -> (D', S) float64: the mean over the images and the tokens of each scale"""
        out, b = [], 0
        for pn in self.patch_nums:
            out.append(x[..., b:b + pn * pn].double().mean(dim=(0, 2)))
            b += pn * pn
        return torch.stack(out, -1)

    def per_scale(self) -> dict:
        """{'nll', 'entropy', 'kl', 'agree', 'acc'}: (D', S) float64 means per layer and scale"""
        return dict(nll=self._scale_mean(self.nll), entropy=self._scale_mean(self.entropy), kl=self._scale_mean(self.kl),
                    agree=self._scale_mean(self.agree()), acc=self.acc())

    def agree(self) -> torch.Tensor:
        """(N, D', L) bool: the layer predicts what the last selected layer predicts"""
        return self.pred == self.pred[:, -1:]

    def settle_depth(self) -> torch.Tensor:
        """(N, L) int64: the first selected layer (a block index) from which pred stays equal to the last selected layer's"""
        a = self.agree().to(torch.int64)
        stays = torch.flip(torch.cumprod(torch.flip(a, (1,)), 1), (1,))                   # agrees here and at every later selected layer
        first = a.shape[1] - stays.sum(1)
        return torch.tensor(self.layers, dtype=torch.int64, device=a.device)[first]

    def acc(self) -> torch.Tensor:
        """(D', S) float64: the share of tokens with rank == 0, per layer and scale"""
        return self._scale_mean(self.rank == 0)

    def __repr__(self):
        N, D, L = self.nll.shape
        return f'LogitLens(images={N}, layers={self.layers}, tokens={L})'


def logit_lens_torch(var, gt: torch.Tensor, label: torch.Tensor, layers: tuple, max_rows: int):
    """VAR.logit_lens's definitions in PyTorch (CPU models, train mode, prog_si >= 0): _forward_torch's pass with a forward hook on every
    selected block, get_logits on each hooked output, and the per-token values from float64 log-softmaxes.  gt (N, L) tokens, label (N,)
    labels -> (nll, entropy, kl fp32, pred int64, rank int32), each (N, D', ed) with ed the tokens _forward_torch covers"""
    ed = var.begin_ends[var.prog_si][1] if var.prog_si >= 0 else var.L
    x_all = var.vae_proxy[0].quantize.idxBl_to_var_input([gt[:, b:e] for b, e in var.begin_ends])[:, :ed - var.first_l]
    final = var.depth - 1
    parts = []
    for i0 in range(0, gt.shape[0], int(max_rows)):
        lab, g = label[i0:i0 + max_rows], gt[i0:i0 + max_rows, :ed]
        caught = {}
        hooks = [var.blocks[bi].register_forward_hook(lambda mod, inp, out, bi=bi: caught.__setitem__(bi, out)) for bi in layers if bi != final]
        try:
            zf = var._forward_torch(lab, x_all[i0:i0 + max_rows]).float()
        finally:
            for h in hooks:
                h.remove()
        cond = var.class_emb(lab)
        lpf = torch.log_softmax(zf.double(), dim=-1)
        pf = lpf.exp()
        per = []
        for bi in layers:
            z = zf if bi == final else var.get_logits(caught[bi].float(), cond).float()
            _, _, pred, rank = token_eval_torch(z, g)
            lp = lpf if bi == final else torch.log_softmax(z.double(), dim=-1)
            p = lp.exp()
            zero = torch.zeros((), dtype=torch.float64, device=z.device)
            ent = -torch.where(p > 0, p * lp, zero).sum(-1)
            kl = torch.where(pf > 0, pf * (lpf - lp), zero).sum(-1)
            per.append(((-lp.gather(-1, g.unsqueeze(-1)).squeeze(-1)).float(), ent.float(), kl.float(), pred, rank))
        parts.append(tuple(torch.stack(f, 1) for f in zip(*per)))
    return tuple(torch.cat(f) for f in zip(*parts))


class LogitAttribution:
    """VAR.logit_attribution's result: the final logit of every token as a sum over what each head and each MLP wrote into the residual stream
    (direct logit attribution), on the model's device.  With a the target token, b' the rival (none: r = W[a]), r = W[a] - W[b'], s and sh the
    head's modulation, sigma the LayerNorm deviation of the final stream x and ghat = (r (1 + s) - mean(r (1 + s))) / sigma:
      value      (N, L) fp32        z_a, or z_a - z_b', read from the real logits row
      konst      (N, L) fp32        r . sh + b_a - b_b'
      embed      (N, L) fp32        ghat . (the stream in front of block 0: first map or word embedding, plus level and position)
      attn, mlp  (N, D', L) fp32    ghat . (what block layers[d]'s attention / MLP branch added to the stream)
      head       (N, D', H, L) fp32 the part of attn that head h wrote;  attn_bias (N, D', L): the part proj's bias wrote
      rest       (N, L) fp32        ghat . x - embed - sum over the selected blocks of (attn + mlp): the blocks `layers` leaves out
      residual   (N, L) fp32        value - (konst + ghat . x): what the fp32 head GEMM and the frozen sigma leave unexplained
      rival      (N, L) int64       b', -1 where there is none (target 'gt', or a token whose target or rival is out of range: its values are NaN)
      layers (the D' block indices), patch_nums: the scales the result covers
    Each fp32 value is rounded once from a float64 quantity.  The methods run in PyTorch with float64 sums."""
    TERMS = ('value', 'konst', 'embed', 'rest', 'residual', 'attn', 'mlp', 'attn_bias', 'head')
    __slots__ = TERMS + ('rival', 'layers', 'patch_nums')

    def __init__(self, layers, patch_nums, rival, **terms):
        self.layers, self.patch_nums, self.rival = tuple(layers), tuple(patch_nums), rival
        for k in self.TERMS:
            setattr(self, k, terms[k])

    def _spans(self) -> list:
        ends = np.cumsum([pn * pn for pn in self.patch_nums]).tolist()
        return list(zip([0] + ends[:-1], ends))

    def head_matrix(self) -> torch.Tensor:
        """(D', H) float64: every head's term, the mean over the images and the tokens"""
        return self.head.double().mean(dim=(0, 3))

    def per_scale(self) -> dict:
        """{term: float64 means over the images and the tokens of each scale, the scale last: (S,), (D', S) or (D', H, S)}"""
        return {k: torch.stack([getattr(self, k)[..., b:e].double().mean(dim=(0, -1)) for b, e in self._spans()], -1) for k in self.TERMS}

    def centered(self) -> 'LogitAttribution':
        """every term minus its mean over the tokens of its scale and image (float64, rounded to fp32 once): the terms relative to the mean
        token of the scale"""
        out = {}
        for k in self.TERMS:
            x = getattr(self, k).double()
            out[k] = torch.cat([x[..., b:e] - x[..., b:e].mean(-1, keepdim=True) for b, e in self._spans()], -1).to(torch.float32)
        return LogitAttribution(self.layers, self.patch_nums, self.rival, **out)

    def completeness(self) -> dict:
        """{'residual': max |residual|, 'heads': max |sum_h head + attn_bias - attn|} as floats, over the tokens whose values are not NaN"""
        gap = self.head.double().sum(2) + self.attn_bias.double() - self.attn.double()
        fin = lambda t: t[~torch.isnan(t)]
        mx = lambda t: float(fin(t).abs().max()) if fin(t).numel() else 0.0
        return dict(residual=mx(self.residual.double()), heads=mx(gap))

    def __repr__(self):
        N, D, H, L = self.head.shape
        return f'LogitAttribution(images={N}, layers={self.layers}, heads={H}, tokens={L})'


def logit_attribution_torch(var, gt: torch.Tensor, label: torch.Tensor, target: str = 'gt', against: Optional[torch.Tensor] = None, layers=None,
                            max_rows: int = 64) -> dict:
    """VAR.logit_attribution's definitions in PyTorch on the module stack (any device; the arithmetic follows the parameters' dtype, float64
    included; prog_si >= 0: the scales 0 .. prog_si): the masked teacher-forced pass with forward hooks on every selected block's attention
    (its branch), on its proj (the input, head by head) and on its MLP.  Unlike the HIP route it takes a branch's term from the hooked branch
    times its gate, not from a difference of streams.  gt (N, L) tokens, label (N,) labels, against None or (N, L) rivals -> the dict of
    LogitAttribution's terms in the parameters' dtype, each over the ed tokens the pass covers, and rival int64.  Dropout and drop path must
    be off (eval mode, or zero rates): the stream is then the plain sum the decomposition needs."""
    ed = var.begin_ends[var.prog_si][1] if var.prog_si >= 0 else var.L
    dt, dev = var.pos_start.dtype, gt.device
    C, H, V = var.C, var.num_heads, var.V
    layers = tuple(range(var.depth)) if layers is None else tuple(layers)
    x_all = var.vae_proxy[0].quantize.idxBl_to_var_input([gt[:, b:e] for b, e in var.begin_ends])[:, :ed - var.first_l].to(dt)
    mask = var.attn_bias_for_masking[:, :, :ed, :ed].to(dt)
    W, bias = var.head.weight, var.head.bias
    eps = var.head_nm.ln_wo_grad.eps
    parts = []
    for i0 in range(0, gt.shape[0], int(max_rows)):
        lab, g = label[i0:i0 + max_rows], gt[i0:i0 + max_rows, :ed]
        B = lab.shape[0]
        caught, hooks = {}, []
        for bi in layers:
            blk = var.blocks[bi]
            hooks += [blk.attn.register_forward_hook(lambda m, i, o, bi=bi: caught.__setitem__(('attn', bi), o)),
                      blk.attn.proj.register_forward_pre_hook(lambda m, i, bi=bi: caught.__setitem__(('att', bi), i[0])),
                      blk.ffn.register_forward_hook(lambda m, i, o, bi=bi: caught.__setitem__(('mlp', bi), o))]
        try:
            cond = var.class_emb(lab)
            sos = cond.unsqueeze(1).expand(B, var.first_l, -1) + var.pos_start.expand(B, var.first_l, -1)
            x = torch.cat((sos, var.word_embed(x_all[i0:i0 + max_rows])), dim=1) if ed > var.first_l else sos
            e = x = x + var.lvl_embed(var.lvl_1L[:, :ed].expand(B, -1)) + var.pos_1LC[:, :ed]
            cgs = var.shared_ada_lin(cond)
            for blk in var.blocks:
                x = blk(x=x, cond_BD=cgs, attn_bias=mask)
        finally:
            for h in hooks:
                h.remove()
        s, sh = var.head_nm.ada_lin(cond).view(-1, 1, 2, C).unbind(2)
        z = var.head(var.head_nm(x, cond))
        za = z.gather(-1, g.unsqueeze(-1)).squeeze(-1)
        ok = ~torch.isnan(z).any(-1)
        if against is not None:
            rival = against[i0:i0 + max_rows, :ed].to(dev, torch.int64)
            ok = ok & (rival >= 0) & (rival < V)
        elif target == 'margin':
            zm = z.masked_fill(torch.nn.functional.one_hot(g, V).bool(), float('-inf'))
            idx = torch.arange(V, device=dev).expand_as(zm)
            rival = torch.where(zm == zm.amax(-1, keepdim=True), idx, torch.full_like(idx, V)).amin(-1)      # the lowest index on ties
            ok = ok & (rival < V)
        else:
            rival = None
        r, kb, value = W[g], bias[g], za
        if rival is not None:
            rb = rival.clamp(0, V - 1)
            r, kb, value = r - W[rb], kb - bias[rb], za - z.gather(-1, rb.unsqueeze(-1)).squeeze(-1)
        gv = r * (1 + s)
        sigma = (x.var(-1, unbiased=False, keepdim=True) + eps).sqrt()
        ghat = (gv - gv.mean(-1, keepdim=True)) / sigma
        dot = lambda a: (ghat * a).sum(-1)
        gx = dot(x)
        o = dict(value=value, konst=(r * sh).sum(-1) + kb, embed=dot(e), attn=[], mlp=[], attn_bias=[], head=[])
        o['residual'] = value - (o['konst'] + gx)
        rest = gx - o['embed']
        for bi in layers:
            blk = var.blocks[bi]
            g1, g2 = blk._six(cgs)[:2]
            o['attn'].append(dot(caught[('attn', bi)] * g1))
            o['mlp'].append(dot(caught[('mlp', bi)] * g2))
            o['attn_bias'].append(dot(blk.attn.proj.bias * g1))
            u = (ghat * g1) @ blk.attn.proj.weight
            o['head'].append((u * caught[('att', bi)]).view(B, ed, H, C // H).sum(-1).transpose(1, 2))
            rest = rest - (o['attn'][-1] + o['mlp'][-1])
        o['rest'] = rest
        for k in ('attn', 'mlp', 'attn_bias', 'head'):
            o[k] = torch.stack(o[k], 1)
        for k in o:
            o[k] = torch.where(ok.view(B, *([1] * (o[k].dim() - 2)), ed), o[k], torch.full_like(o[k], float('nan')))
        o['rival'] = torch.full_like(g, -1) if rival is None else torch.where(ok, rival, torch.full_like(rival, -1))
        parts.append(o)
    return {k: torch.cat([p[k] for p in parts]) for k in parts[0]}


class PatchEffects:
    """VAR.patch_effects' result: what an image's prediction loses when a head, an attention layer or an MLP is ablated or patched, per token,
    on the model's device.  Index 0 of the second axis is the clean row, index j + 1 the row with the intervention sites[j]; with z the row's
    fp32 logits, p their softmax and pc the clean row's softmax:
      nll      (N, P + 1, L) fp32   -log p[gt]                       (index 0: VAR.evaluate's nll_BL)
      entropy  (N, P + 1, L) fp32   -sum_v p_v log p_v, in nats
      kl       (N, P + 1, L) fp32   KL(pc || p) = sum_v pc_v (log pc_v - log p_v); exactly 0 at index 0
      pred     (N, P + 1, L) int64  argmax z;  rank (N, P + 1, L) int32: |{v : z_v > z_gt or (z_v == z_gt and v < gt)}|
      sites: the P entries, each a tuple of elementary sites ('head', layer, head) | ('attn', layer) | ('mlp', layer); mode, scales (the
      scale indices at which the interventions applied), patch_nums (the scales the result covers), depth and num_heads of the model
    The methods run in PyTorch with float64 sums."""
    __slots__ = ('sites', 'mode', 'scales', 'nll', 'entropy', 'kl', 'pred', 'rank', 'patch_nums', 'depth', 'num_heads')

    def __init__(self, sites, mode, scales, nll, entropy, kl, pred, rank, patch_nums, depth, num_heads):
        self.sites, self.mode, self.scales, self.patch_nums = tuple(sites), mode, tuple(scales), tuple(patch_nums)
        self.nll, self.entropy, self.kl, self.pred, self.rank = nll, entropy, kl, pred, rank
        self.depth, self.num_heads = int(depth), int(num_heads)

    def effect(self) -> torch.Tensor:
        """(N, P, L) fp32: the loss a site's intervention adds, nll[:, 1:] - nll[:, :1]"""
        return self.nll[:, 1:] - self.nll[:, :1]

    def _scale_mean(self, x: torch.Tensor) -> torch.Tensor:
        """x (N, P, L) -> (P, S) float64: the mean over the images and the tokens of each scale"""
        out, b = [], 0
        for pn in self.patch_nums:
            out.append(x[..., b:b + pn * pn].double().mean(dim=(0, 2)))
            b += pn * pn
        return torch.stack(out, -1)

    def per_scale(self) -> dict:
        """{'effect', 'kl'}: (P, S) float64 means per site and scale"""
        return dict(effect=self._scale_mean(self.effect()), kl=self._scale_mean(self.kl[:, 1:]))

    def head_matrix(self) -> torch.Tensor:
        """(depth, H) float64: the mean effect of every site that is one single head, NaN where a head was not asked for (a head asked for
        more than once: its last entry)"""
        m = torch.full((self.depth, self.num_heads), float('nan'), dtype=torch.float64, device=self.nll.device)
        mean = self.effect().double().mean(dim=(0, 2))
        for j, group in enumerate(self.sites):
            if len(group) == 1 and group[0][0] == 'head':
                m[group[0][1], group[0][2]] = mean[j]
        return m

    def __repr__(self):
        N, P1, L = self.nll.shape
        return f'PatchEffects(images={N}, sites={P1 - 1}, mode={self.mode!r}, tokens={L})'


def patch_effects_torch(var, gt: torch.Tensor, label: torch.Tensor, columns: tuple, mode: str, donor: Optional[torch.Tensor], scales: tuple, _tap=None):
    """VAR.patch_effects' definitions in PyTorch on the module stack (CPU models, train mode, prog_si >= 0; the arithmetic follows the parameters'
    dtype): one masked teacher-forced pass per row, a manual block loop that rewrites the attention output in front of proj and the MLP hidden
    activation behind the GELU.  gt (N, L) tokens, label (N,) labels, columns: per site the (matrix 'att' | 'hid', block, c0, c1) ranges
    (args.patch_columns), donor (N,) labels or None, scales: the scale indices at which the interventions apply -> (nll, entropy, kl float64,
    pred int64, rank int32), each (N, P + 1, ed) with ed the tokens the pass covers.  'zero' writes 0, 'mean' the mean over the tokens of the
    scale (per scale, row and column), 'donor' the activation of a pass on the same tokens under the donor label.  Every row is a pass of its
    own with batch size 1, so a row's values do not depend on its neighbours; dropout and drop path are not applied (the deterministic pass).
    _tap (tests): called with (image, row index, the row's logits (ed, V)) for every row."""
    F = torch.nn.functional
    ed = var.begin_ends[var.prog_si][1] if var.prog_si >= 0 else var.L
    dt = var.pos_start.dtype
    mask = var.attn_bias_for_masking[:, :, :ed, :ed].to(dt)
    spans = [var.begin_ends[si] for si in scales if var.begin_ends[si][1] <= ed]
    x_in = lambda n: var.vae_proxy[0].quantize.idxBl_to_var_input([gt[n:n + 1, b:e] for b, e in var.begin_ends])[:, :ed - var.first_l].to(dt)

    def run(n, lab, group, acts, record):
        """the logits (ed, V) of image n under label lab with the column ranges of `group` rewritten; record: keep every activation in acts"""
        todo = {}
        for kind, bi, c0, c1 in group:
            todo.setdefault((bi, kind), []).append((c0, c1))

        def rewrite(a, key):
            if record:
                acts[key] = a
            if key not in todo:
                return a
            a = a.clone()
            for c0, c1 in todo[key]:
                for b, e in spans:
                    a[:, b:e, c0:c1] = 0 if mode == 'zero' else a[:, b:e, c0:c1].mean(1, keepdim=True) if mode == 'mean' else acts[key][:, b:e, c0:c1]
            return a
        cond = var.class_emb(lab.view(1))
        sos = cond.unsqueeze(1).expand(1, var.first_l, -1) + var.pos_start.expand(1, var.first_l, -1)
        x = torch.cat((sos, var.word_embed(xs[n])), dim=1) if ed > var.first_l else sos
        x = x + var.lvl_embed(var.lvl_1L[:, :ed].expand(1, -1)) + var.pos_1LC[:, :ed]
        cond_or_gss = var.shared_ada_lin(cond)
        for bi, blk in enumerate(var.blocks):
            at = blk.attn
            gamma1, gamma2, scale1, scale2, shift1, shift2 = blk._six(cond_or_gss)
            q, k, v = at._heads(blk.ln_wo_grad(x) * (scale1 + 1) + shift1)
            if at.attn_l2_norm:
                q, k = F.normalize(q, dim=-1) * at.scale_mul_1H11.clamp_max(at.max_scale_mul).exp(), F.normalize(k, dim=-1)
            ctx = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, scale=at.scale).transpose(1, 2).reshape(1, ed, var.C)
            x = x + at.proj(rewrite(ctx, (bi, 'att'))) * gamma1
            hid = blk.ffn.act(blk.ffn.fc1(blk.ln_wo_grad(x) * (scale2 + 1) + shift2))
            x = x + blk.ffn.fc2(rewrite(hid, (bi, 'hid'))) * gamma2
        return var.head(var.head_nm(x, cond))[0]

    zero = torch.zeros((), dtype=torch.float64, device=gt.device)
    rows, xs = [], {}
    for n in range(gt.shape[0]):
        acts = {}
        xs = {n: x_in(n)}                                       # (an image's input on its own: the interpolation is not batch-invariant either)
        if mode == 'donor':
            run(n, donor[n], (), acts, True)
        g = gt[n, :ed]
        per, lpc = [], None
        for group in ((),) + tuple(columns):
            z = run(n, label[n], group, acts, False)
            if _tap is not None:
                _tap(n, len(per), z)
            lp = torch.log_softmax(z.double(), dim=-1)
            lpc = lp if lpc is None else lpc
            p, pc = lp.exp(), lpc.exp()
            _, _, pred, rank = token_eval_torch(z.float().unsqueeze(0), g.unsqueeze(0))
            per.append((-lp.gather(-1, g.unsqueeze(-1)).squeeze(-1), -torch.where(p > 0, p * lp, zero).sum(-1),
                        torch.where(pc > 0, pc * (lpc - lp), zero).sum(-1), pred[0], rank[0]))
        rows.append(tuple(torch.stack(f) for f in zip(*per)))
    return tuple(torch.stack(f) for f in zip(*rows))


class AttentionKnockout:
    """VAR.attention_knockout's result: what an image's prediction loses when queries of one scale may not read the keys of another, per token, on
    the model's device.  Index 0 of the second axis is the clean row, index j + 1 the row with the cut edges[j]; with z the row's fp32 logits,
    p their softmax and pc the clean row's softmax:
      nll      (N, P + 1, L) fp32   -log p[gt]                       (index 0: VAR.evaluate's nll_BL)
      entropy  (N, P + 1, L) fp32   -sum_v p_v log p_v, in nats
      kl       (N, P + 1, L) fp32   KL(pc || p) = sum_v pc_v (log pc_v - log p_v); exactly 0 at index 0
      pred     (N, P + 1, L) int64  argmax z;  rank (N, P + 1, L) int32: |{v : z_v > z_gt or (z_v == z_gt and v < gt)}|
      edges: the P entries, each a tuple of elementary edges (q, k, blocks, heads): queries of scale q do not see the keys of scale k in those
      blocks and heads; layers, heads (the call's), patch_nums (the scales the result covers)
    The methods run in PyTorch with float64 sums."""
    __slots__ = ('edges', 'layers', 'heads', 'nll', 'entropy', 'kl', 'pred', 'rank', 'patch_nums')

    def __init__(self, edges, layers, heads, nll, entropy, kl, pred, rank, patch_nums):
        self.edges, self.layers, self.heads, self.patch_nums = tuple(edges), tuple(layers), tuple(heads), tuple(patch_nums)
        self.nll, self.entropy, self.kl, self.pred, self.rank = nll, entropy, kl, pred, rank

    def effect(self) -> torch.Tensor:
        """(N, P, L) fp32: the loss an entry's cut adds, nll[:, 1:] - nll[:, :1]"""
        return self.nll[:, 1:] - self.nll[:, :1]

    def _begins(self) -> list:
        b = [0]
        for pn in self.patch_nums:
            b.append(b[-1] + pn * pn)
        return b

    def per_scale(self) -> dict:
        """{'effect', 'kl'}: (P, S) float64 means per entry and token scale, over the images and the scale's tokens"""
        b = self._begins()
        mean = lambda x: torch.stack([x[..., b[s]:b[s + 1]].double().mean(dim=(0, 2)) for s in range(len(self.patch_nums))], -1)
        return dict(effect=mean(self.effect()), kl=mean(self.kl[:, 1:]))

    def edge_matrix(self, at: str = 'query') -> torch.Tensor:
        """(S, S) float64, [q, k]: the mean added loss of every entry that is one single edge (q, k), over the images and the tokens of scale q
        (at='query') or the tokens of scale q and every later scale (at='all'); NaN where no entry exists (an edge asked for more than once:
        its last entry)"""
        if at not in ('query', 'all'):
            raise ValueError(f"at must be 'query' or 'all', got {at!r}")
        S, b = len(self.patch_nums), self._begins()
        m = torch.full((S, S), float('nan'), dtype=torch.float64, device=self.nll.device)
        eff = self.effect().double()
        for j, group in enumerate(self.edges):
            if len(group) == 1 and group[0][0] < S:
                q, k = group[0][:2]
                m[q, k] = eff[:, j, b[q]:(b[q + 1] if at == 'query' else b[S])].mean()
        return m

    def __repr__(self):
        N, P1, L = self.nll.shape
        return f'AttentionKnockout(images={N}, edges={P1 - 1}, tokens={L})'


def attention_knockout_torch(var, gt: torch.Tensor, label: torch.Tensor, cuts: tuple, _tap=None):
    """VAR.attention_knockout's definitions in PyTorch on the module stack (CPU models, train mode, prog_si >= 0; the arithmetic follows the
    parameters' dtype): one masked teacher-forced pass per row with batch size 1, a manual block loop whose attention takes, on top of the
    block-causal mask, an additive bias per head that is -inf where the row's cut hides a key scale from a query scale.  gt (N, L) tokens,
    label (N,) labels, cuts: per entry {(query scale, block): the H key-scale masks} (args.knockout_masks) -> (nll, entropy, kl float64, pred
    int64, rank int32), each (N, P + 1, ed) with ed the tokens the pass covers.  A row's values do not depend on its neighbours; dropout and
    drop path are not applied (the deterministic pass).  _tap (tests): called with (image, row index, the row's logits (ed, V)) for every row."""
    F = torch.nn.functional
    ed = var.begin_ends[var.prog_si][1] if var.prog_si >= 0 else var.L
    dt = var.pos_start.dtype
    H = var.num_heads
    mask = var.attn_bias_for_masking[:, :, :ed, :ed].to(dt)

    def bias_of(cut, bi):
        """(1, H, ed, ed): the block-causal mask with the block's hidden (query scale, key scale) rectangles at -inf, or the mask itself"""
        todo = [(si, masks) for (si, b), masks in cut.items() if b == bi and var.begin_ends[si][1] <= ed]
        if not todo:
            return mask
        bias = mask.expand(1, H, ed, ed).clone()
        for si, masks in todo:
            bq, eq = var.begin_ends[si]
            for h, m in enumerate(masks):
                for k in range(si + 1):
                    if not (m >> k) & 1:
                        bk, ek = var.begin_ends[k]
                        bias[0, h, bq:eq, bk:ek] = float('-inf')
        return bias

    def run(lab, x_in, cut):
        cond = var.class_emb(lab.view(1))
        sos = cond.unsqueeze(1).expand(1, var.first_l, -1) + var.pos_start.expand(1, var.first_l, -1)
        x = torch.cat((sos, var.word_embed(x_in)), dim=1) if ed > var.first_l else sos
        x = x + var.lvl_embed(var.lvl_1L[:, :ed].expand(1, -1)) + var.pos_1LC[:, :ed]
        cond_or_gss = var.shared_ada_lin(cond)
        for bi, blk in enumerate(var.blocks):
            at = blk.attn
            gamma1, gamma2, scale1, scale2, shift1, shift2 = blk._six(cond_or_gss)
            q, k, v = at._heads(blk.ln_wo_grad(x) * (scale1 + 1) + shift1)
            if at.attn_l2_norm:
                q, k = F.normalize(q, dim=-1) * at.scale_mul_1H11.clamp_max(at.max_scale_mul).exp(), F.normalize(k, dim=-1)
            ctx = F.scaled_dot_product_attention(q, k, v, attn_mask=bias_of(cut, bi), scale=at.scale).transpose(1, 2).reshape(1, ed, var.C)
            x = x + at.proj(ctx) * gamma1
            x = x + blk.ffn.fc2(blk.ffn.act(blk.ffn.fc1(blk.ln_wo_grad(x) * (scale2 + 1) + shift2))) * gamma2
        return var.head(var.head_nm(x, cond))[0]

    zero = torch.zeros((), dtype=torch.float64, device=gt.device)
    rows = []
    for n in range(gt.shape[0]):
        # (an image's input on its own: the quantizer's interpolation is not batch-invariant)
        x_in = var.vae_proxy[0].quantize.idxBl_to_var_input([gt[n:n + 1, b:e] for b, e in var.begin_ends])[:, :ed - var.first_l].to(dt)
        g = gt[n, :ed]
        per, lpc = [], None
        for cut in ({},) + tuple(cuts):
            z = run(label[n], x_in, cut)
            if _tap is not None:
                _tap(n, len(per), z)
            lp = torch.log_softmax(z.double(), dim=-1)
            lpc = lp if lpc is None else lpc
            p, pc = lp.exp(), lpc.exp()
            _, _, pred, rank = token_eval_torch(z.float().unsqueeze(0), g.unsqueeze(0))
            per.append((-lp.gather(-1, g.unsqueeze(-1)).squeeze(-1), -torch.where(p > 0, p * lp, zero).sum(-1),
                        torch.where(pc > 0, pc * (lpc - lp), zero).sum(-1), pred[0], rank[0]))
        rows.append(tuple(torch.stack(f) for f in zip(*per)))
    return tuple(torch.stack(f) for f in zip(*rows))


class EvidenceMaps:
    """VAR.evidence_maps' result: where in the image the evidence for each class sits.  With m[n, k, y, x] the map of class k (the selected
    scales' per-token scores, each resampled bilinearly to size x size and weighted by its share of the selected tokens):
      lo, hi     (N,) fp32: min and max of m over all classes and pixels of image n (the fork's global normalisation)
      pred       (N, size, size) int32: the class with the largest m at the pixel, the lowest index among exact ties
      margin     (N, size, size) fp32: largest minus second largest m (+inf with one class)
      area       (N, K) int32: pixels won by each class (sums to size^2)
      maps       (N, K, size, size) fp32 or None (return_maps=True)
      overlays   (N, K, size, size, 3) uint8 or None (an image was given): the fork's jet overlay of every class map
      scales, size, patch_nums: what the result covers
    A (K, L) input gives N = 1."""
    __slots__ = ('lo', 'hi', 'pred', 'margin', 'area', 'maps', 'overlays', 'scales', 'size', 'patch_nums')

    def __init__(self, lo, hi, pred, margin, area, maps, overlays, scales, size, patch_nums):
        self.lo, self.hi, self.pred, self.margin, self.area, self.maps, self.overlays = lo, hi, pred, margin, area, maps, overlays
        self.scales, self.size, self.patch_nums = tuple(scales), int(size), tuple(patch_nums)

    def normalized(self) -> torch.Tensor:
        """(maps - lo) / (hi - lo) per image in fp32, maps - lo where hi == lo: what the colour table is indexed with (needs return_maps=True)"""
        if self.maps is None:
            raise ValueError('normalized() needs the maps: call evidence_maps(..., return_maps=True)')
        return _evidence_normalize(self.maps, self.lo, self.hi)

    def __repr__(self):
        N, K = self.area.shape
        return (f'EvidenceMaps(images={N}, classes={K}, size={self.size}, scales={self.scales}, maps={self.maps is not None}, '
                f'overlays={self.overlays is not None})')


def _evidence_normalize(maps: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor) -> torch.Tensor:
    rng = (hi - lo).view(-1, 1, 1, 1)
    v = maps - lo.view(-1, 1, 1, 1)
    return torch.where(rng != 0, v / rng, v)


_JET = []


def jet_table() -> torch.Tensor:
    """(256, 3) uint8: matplotlib's 'jet' as (lut * 255).astype(uint8), the table the overlay kernel holds (read from the library: one copy)"""
    if not _JET:
        from .. import hip
        t = np.zeros(768, np.uint8)
        hip.call_host('evidence_jet_host', t)
        _JET.append(torch.from_numpy(t.reshape(256, 3)))
    return _JET[0]


def evidence_maps_torch(scores: torch.Tensor, patch_nums, scales, size: int, image: Optional[torch.Tensor] = None, image_pm1: bool = True,
                        alpha: float = 0.5, return_maps: bool = False) -> dict:
    """VAR.evidence_maps' definitions in PyTorch, in the operation order of the kernels: the twin the GPU is held to bit for
    bit.  scores: (N, K, L) fp32, image: (N, 3, size, size) fp32 or None -> dict(lo, hi, pred, margin, area, maps | None, overlays | None).
    Every product and sum is its own fp32 operation (separate mul / add calls: nothing here may be fused); the (N, K, size, size) maps are
    materialised, which is what the kernels avoid."""
    from ..engine import bilinear_axis, evidence_scales
    N, K, L = scores.shape
    dev = scores.device
    pn, begin, w = evidence_scales(patch_nums, scales)
    m = torch.zeros(N, K, size, size, dtype=torch.float32, device=dev)
    one = torch.ones((), dtype=torch.float32, device=dev)
    for p, b, ws in zip(pn.tolist(), begin.tolist(), w):
        i0, i1, l1 = (torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in bilinear_axis(p, size))
        i0, i1 = i0.long(), i1.long()
        l0 = torch.sub(one, l1)
        g = scores[:, :, b:b + p * p].reshape(N, K, p, p)
        r0, r1 = g[:, :, i0], g[:, :, i1]                                  # (N, K, size, p): the rows y.i0 and y.i1
        l0x, l1x, l0y, l1y = l0.view(1, 1, 1, -1), l1.view(1, 1, 1, -1), l0.view(1, 1, -1, 1), l1.view(1, 1, -1, 1)
        top = torch.add(torch.mul(l0x, r0[..., i0]), torch.mul(l1x, r0[..., i1]))
        bot = torch.add(torch.mul(l0x, r1[..., i0]), torch.mul(l1x, r1[..., i1]))
        v = torch.add(torch.mul(l0y, top), torch.mul(l1y, bot))
        m = torch.add(m, torch.mul(v, torch.tensor(ws, dtype=torch.float32, device=dev)))
    lo, hi = m.amin((1, 2, 3)), m.amax((1, 2, 3))
    best = m.amax(1)
    ks = torch.arange(K, device=dev).view(1, K, 1, 1)
    pred = torch.where(m == best.unsqueeze(1), ks, K - 1).amin(1)          # the lowest index among exact ties (no match: a NaN under check=False)
    second = m.masked_fill(ks == pred.unsqueeze(1), -math.inf).amax(1)
    area = torch.stack([torch.bincount(pred[n].reshape(-1), minlength=K) for n in range(N)]).to(torch.int32)
    out = dict(lo=lo, hi=hi, pred=pred.to(torch.int32), margin=torch.sub(best, second), area=area, maps=m if return_maps else None, overlays=None)
    if image is not None:
        jet = jet_table().to(dev)
        x = image.float()
        if image_pm1:
            x = torch.div(torch.add(x, 1.0), 2.0)
        g8 = torch.mul(x, 255.0).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).double()       # truncated, as numpy's astype
        over = torch.empty(N, K, size, size, 3, dtype=torch.uint8, device=dev)
        for n in range(N):
            v = _evidence_normalize(m[n:n + 1], lo[n:n + 1], hi[n:n + 1])[0]
            col = jet[torch.mul(v, 256.0).clamp(0, 255).long()].double()                          # min(int(v * 256), 255)
            o = torch.add(torch.mul(g8[n].unsqueeze(0), 1.0 - float(alpha)), torch.mul(col, float(alpha)))
            over[n] = o.clamp(0, 255).to(torch.uint8)
        out['overlays'] = over
    return out


def evidence_maps(scores, patch_nums, *, scales=None, size: int = 256, image=None, image_range: str = 'pm1', alpha: float = 0.5,
                  return_maps: bool = False, check: bool = True) -> EvidenceMaps:
    """VAR.evidence_maps for any patch_nums (the method passes the model's): see there."""
    patch_nums = tuple(int(p) for p in patch_nums)
    S, L = len(patch_nums), sum(p * p for p in patch_nums)
    if not isinstance(scores, torch.Tensor) or scores.dtype != torch.float32 or scores.dim() not in (2, 3) or scores.shape[-1] != L \
            or scores.numel() == 0:
        raise ValueError(f'scores must be a (N, K, {L}) or (K, {L}) fp32 tensor with N, K >= 1')
    s3 = scores.detach().reshape(-1, scores.shape[-2], L).contiguous() if scores.dim() == 3 else scores.detach().reshape(1, -1, L).contiguous()
    N, K = s3.shape[:2]
    if scales is None:
        scales = tuple(range(S // 2))
    try:
        scales = tuple(scales)
        ok = all(isinstance(s, (int, np.integer)) and not isinstance(s, bool) for s in scales)
    except TypeError:
        ok = False
    if not ok or len(scales) == 0 or any(not 0 <= s < S for s in scales) or any(b <= a for a, b in zip(scales, scales[1:])):
        raise ValueError(f'scales must be a non-empty increasing sequence of scale indices in [0, {S})')
    scales = tuple(int(s) for s in scales)
    if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or not 1 <= size <= 4096:
        raise ValueError('size must be an integer in [1, 4096]')
    size = int(size)
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float, np.integer, np.floating)) or not 0.0 <= float(alpha) <= 1.0:
        raise ValueError('alpha must be a number in [0, 1]')
    if image_range not in ('pm1', '01'):
        raise ValueError("image_range must be 'pm1' (the image is in [-1, 1]) or '01'")
    if image is not None:
        if not isinstance(image, torch.Tensor) or not image.is_floating_point() or image.dim() not in (3, 4) \
                or tuple(image.shape[-3:]) != (3, size, size) or (image.dim() == 4 and image.shape[0] != N) or (image.dim() == 3 and N != 1):
            raise ValueError(f'image must be a ({N}, 3, {size}, {size}) floating-point tensor' + (f' or (3, {size}, {size})' if N == 1 else ''))
        image = image.detach().to(s3.device, torch.float32).reshape(N, 3, size, size).contiguous()
    if check:
        sel = [s3[:, :, sum(p * p for p in patch_nums[:s]):sum(p * p for p in patch_nums[:s + 1])] for s in scales]
        if not bool(torch.isfinite(torch.cat(sel, -1) if len(sel) > 1 else sel[0]).all()):
            raise ValueError('scores of the selected scales must be finite (check=False skips this test: the result is then undefined)')
    if s3.is_cuda:
        from ..engine import evidence_maps_hip
        r = evidence_maps_hip(s3, patch_nums, scales, size, image, image_range == 'pm1', float(alpha), bool(return_maps))
    else:
        r = evidence_maps_torch(s3, patch_nums, scales, size, image, image_range == 'pm1', float(alpha), bool(return_maps))
    return EvidenceMaps(r['lo'], r['hi'], r['pred'], r['margin'], r['area'], r['maps'], r['overlays'], scales, size, patch_nums)


GENERATIVE_FEATURES = ('vae_post', 'vae_fhat')


class SampleRecord:
    """What a scored sampling call returns (VAR.autoregressive_infer_cfg_scored, ..._per_image_scored, sample_best_of), on the model's device:
      images       (B, 3, H, W) fp32 in [0, 1], or None (decode=False)
      tokens       (B, L) int64, the drawn tokens
      logp_cond    (B, L) fp32: log p(token) under the conditional logits (VAR.token_log_likelihood's value at cfg 0 for the same row)
      logp_guided  (B, L) fp32: the same under the guided logits (1 + t) * cond - t * uncond, t = cfg * scale / (S - 1)
      logp_drawn   (B, L) fp32: the same under the distribution the token was drawn from (after top-k / top-p)
      entropy      (B, L) fp32: the entropy of the guided distribution in nats
      kept         (B, L) int32: how many codes top-k / top-p left to draw from
      patch_nums   the scales the L tokens are laid out in
    The definitions, roundings and summation orders are those of varhip_sample_stats_f32 (include/var_hip.h)."""
    __slots__ = ('images', 'tokens', 'logp_cond', 'logp_guided', 'logp_drawn', 'entropy', 'kept', 'patch_nums')
    FIELDS = ('logp_cond', 'logp_guided', 'logp_drawn', 'entropy', 'kept')

    def __init__(self, images, tokens, logp_cond, logp_guided, logp_drawn, entropy, kept, patch_nums):
        self.images, self.tokens, self.logp_cond, self.logp_guided, self.logp_drawn = images, tokens, logp_cond, logp_guided, logp_drawn
        self.entropy, self.kept, self.patch_nums = entropy, kept, tuple(patch_nums)

    def _cum(self, field: str) -> np.ndarray:
        if field not in self.FIELDS:
            raise ValueError(f'field must be one of {self.FIELDS}, got {field!r}')
        return np.add.accumulate(getattr(self, field).detach().cpu().numpy().astype(np.float64), axis=1)      # sequential, in token order

    def per_scale(self) -> dict:
        """{field: (B, S) float64 (a CPU tensor)}: per image and scale the sum over the scale's tokens, added on the host in token order"""
        out = {}
        for field in self.FIELDS:
            x = getattr(self, field).detach().cpu().numpy().astype(np.float64)
            cols, b = [], 0
            for pn in self.patch_nums:
                cols.append(np.add.accumulate(x[:, b:b + pn * pn], axis=1)[:, -1])
                b += pn * pn
            out[field] = torch.from_numpy(np.stack(cols, axis=1))
        return out

    def total(self, field: str) -> torch.Tensor:
        """(B,) float64 (a CPU tensor): the sum of `field` over an image's L tokens, one addition per token in token order (what sample_best_of
        ranks by: varhip_class_select_f32 adds in the same order)"""
        return torch.from_numpy(self._cum(field)[:, -1].copy())

    def __repr__(self):
        B, L = tuple(self.tokens.shape)
        tot = lambda f: '[' + ', '.join(f'{v:.2f}' for v in self.total(f).tolist()[:4]) + (', ...' if B > 4 else '') + ']'
        img = None if self.images is None else tuple(self.images.shape)
        if self.kept is None:                    # (sample_controlled off the HIP path: tokens and images only)
            return f'SampleRecord(B={B}, L={L}, images={img}, no per-token statistics)'
        return (f'SampleRecord(B={B}, L={L}, images={img}, logp_cond={tot("logp_cond")}, logp_guided={tot("logp_guided")}, '
                f'logp_drawn={tot("logp_drawn")}, mean kept={float(self.kept.float().mean()):.1f})')


BEST_OF_FIELDS = ('logp_cond', 'logp_guided', 'logp_drawn')


class NoiseRecord:
    """What VAR.abduct_noise returns: the sampler's noise behind given tokens, on the model's device.
      noise        (B, L, V) fp32: under it the unfiltered guided sampler of (label_src, cfg) draws the tokens; L * V * 4 bytes per image
      logp_src     (B, L) fp32: log p(token) under the guided source distribution, NaN on scales below first_scale, -inf where unreachable
      unreachable  (B, L) bool: no noise explains the token (probability 0 under the source distribution, or a NaN row): the row holds
                   prior noise and a replay is free to draw another token there
      cfg          the B source cfg values;  first_scale: the first abducted scale;  precision: the arithmetic the logits were computed in
    A record belongs to the weights and the precision it was made with (VAR.counterfactual checks both)."""
    __slots__ = ('noise', 'logp_src', 'unreachable', 'cfg', 'first_scale', 'precision', '_sig')

    def __init__(self, noise, logp_src, unreachable, cfg, first_scale, precision, sig):
        self.noise, self.logp_src, self.unreachable, self.cfg = noise, logp_src, unreachable, tuple(cfg)
        self.first_scale, self.precision, self._sig = int(first_scale), precision, sig

    def __repr__(self):
        B, L, V = tuple(self.noise.shape)
        return (f'NoiseRecord(B={B}, L={L}, V={V}, first_scale={self.first_scale}, precision={self.precision!r}, '
                f'unreachable={int(self.unreachable.sum())}, {self.noise.numel() * 4 / 1e6:.1f} MB)')


class CounterfactualResult:
    """What VAR.counterfactual returns, on the model's device; request (b, k) is image b replayed under label_dst[b, k]:
      images       (B, K, 3, H, W) fp32 in [0, 1], or None (decode=False)
      tokens       (B, K, L) int64;  changed (B, K, L) bool: tokens != the given ones
      first_changed_scale  (B, K) int64: the first scale holding a changed token, S where nothing changed
      logp_src, unreachable  (B, L): the NoiseRecord's
      record       the replay's SampleRecord over the B * K requests (row b * K + k); scales below first_scale were not sampled:
                   their log-probabilities and entropy are NaN, kept is 0
      noise        the NoiseRecord the replay read (pass it as noise= to replay again without a second abduction)"""
    __slots__ = ('images', 'tokens', 'changed', 'first_changed_scale', 'logp_src', 'unreachable', 'record', 'noise', 'patch_nums')

    def __init__(self, images, tokens, changed, first_changed_scale, logp_src, unreachable, record, noise, patch_nums):
        self.images, self.tokens, self.changed, self.first_changed_scale = images, tokens, changed, first_changed_scale
        self.logp_src, self.unreachable, self.record, self.noise, self.patch_nums = logp_src, unreachable, record, noise, tuple(patch_nums)

    def change_rate(self) -> torch.Tensor:
        """(B, K, S) float64 (a CPU tensor): per request and scale the share of its tokens that changed"""
        c = self.changed.detach().cpu().numpy()
        cols, b = [], 0
        for pn in self.patch_nums:
            cols.append(c[:, :, b:b + pn * pn].mean(axis=2, dtype=np.float64))
            b += pn * pn
        return torch.from_numpy(np.stack(cols, axis=2))

    def __repr__(self):
        B, K, L = tuple(self.tokens.shape)
        return (f'CounterfactualResult(B={B}, K={K}, L={L}, images={None if self.images is None else tuple(self.images.shape)}, '
                f'changed={float(self.changed.float().mean()):.3f}, unreachable={int(self.unreachable.sum())})')


class ComposedRecord:
    """What VAR.sample_composed returns, on the model's device (coef on the host):
      images       (B, 3, H, W) fp32 in [0, 1], or None (decode=False)
      tokens       (B, L) int64, the drawn tokens
      logp_class   (B, K + 1, L) fp32: log p(token) under each class row's own logits, the unconditional row last (VAR.token_log_likelihood's
                   value at cfg 0 for the same row)
      logp_guided  (B, L) fp32: the same under the mixed row x = sum_k a_k c_k - a_u u
      logp_drawn   (B, L) fp32: the same under the distribution the token was drawn from (x after top-k / top-p)
      entropy      (B, L) fp32: the entropy of softmax(x) in nats
      kept         (B, L) int32: how many codes top-k / top-p left to draw from
      coef         (S, B, K + 1) float32 ndarray: the coefficients (a_1 .. a_K, a_u) used at each scale (var_amd.engine.compose_tables)
      labels       (B, K) int64, as given;  patch_nums: the scales the L tokens are laid out in
    logp_guided, logp_drawn, entropy and kept are SampleRecord's, with the mixed row as the guided row (DESIGN.md sections 26 and 34)."""
    __slots__ = ('images', 'tokens', 'logp_class', 'logp_guided', 'logp_drawn', 'entropy', 'kept', 'coef', 'labels', 'patch_nums')

    def __init__(self, images, tokens, logp_class, logp_guided, logp_drawn, entropy, kept, coef, labels, patch_nums):
        self.images, self.tokens, self.logp_class, self.logp_guided, self.logp_drawn = images, tokens, logp_class, logp_guided, logp_drawn
        self.entropy, self.kept, self.coef, self.labels, self.patch_nums = entropy, kept, coef, labels, tuple(patch_nums)

    def __repr__(self):
        B, G, L = tuple(self.logp_class.shape)
        img = None if self.images is None else tuple(self.images.shape)
        return f'ComposedRecord(B={B}, K={G - 1}, L={L}, images={img}, mean kept={float(self.kept.float().mean()):.1f})'


def rule_order(totals: np.ndarray) -> np.ndarray:
    """indices of a 1-D float64 array in VAR.classify's order: higher total first, NaN below everything, equal totals by lower index"""
    nan = np.isnan(totals)
    return np.lexsort((np.arange(totals.shape[0]), np.where(nan, 0.0, -totals), nan))


def classify_rule(tokens: np.ndarray, ends, schedule) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """VAR.classify applied to full per-token scores (N, K, L) fp32: ends[s] the token end of scale s, schedule [(s, m), ...] ascending.
    -> (pred, total, depth, tokens with the entries past each candidate's depth set to NaN)"""
    N, K, L = tokens.shape
    S = len(ends)
    cum = np.add.accumulate(tokens.astype(np.float64), axis=-1)          # sequential, in token order
    depth = np.full((N, K), S - 1, dtype=np.int64)
    pred = np.empty(N, dtype=np.int64)
    for n in range(N):
        alive = np.arange(K)
        for s, m in schedule:
            order = rule_order(cum[n, alive, ends[s] - 1])
            depth[n, alive[order[m:]]] = s
            alive = np.sort(alive[order[:m]])
        pred[n] = alive[rule_order(cum[n, alive, L - 1])[0]]
    end = np.asarray(ends)[depth]
    total = np.take_along_axis(cum, (end - 1)[..., None], -1)[..., 0]
    out = np.where(np.arange(L) < end[..., None], tokens, np.float32(np.nan)).astype(np.float32)
    return pred, total, depth, out


def get_edit_mask(patch_nums, y0: float, x0: float, y1: float, x1: float, device, inpainting: bool = True) -> torch.Tensor:
    """(P, P) fp32 box mask of the editing notebook (demo_zero_shot_edit.ipynb cell 2), P = patch_nums[-1]: rows round(y0*P):round(y1*P) and
    columns round(x0*P):round(x1*P) (Python round) are 1, the rest 0 — out-painting keeps the box; inpainting=True returns 1 - that (the box
    is generated, the rest kept).  1 keeps the input token, 0 generates a new one (VAR.autoregressive_infer_cfg_with_mask)."""
    P = patch_nums[-1]
    m = torch.zeros(P, P, device=device)
    m[round(y0 * P):round(y1 * P), round(x0 * P):round(x1 * P)] = 1
    return 1 - m if inpainting else m


class VarCodecError(Exception):
    """a blob that VAR.decompress could not turn back into its tokens.  .image: the blob's index in the call; .check: 'bounds' (the decoder
    read past the stream's words or met a slot no symbol owns), 'end' (after the last token the coder's state is not 2^31 or words are left
    over), 'hash' (the tokens' hash differs from the header's) or 'table' (a logits row of the model was refused: NaN or no finite maximum).
    Decoding with other weights than the encoder's ends here too, as a rule at 'end'."""
    def __init__(self, image: int, check: str, detail: str):
        super().__init__(f'decompress: image {image} failed the {check} check: {detail}')
        self.image, self.check = image, check


class CompressResult(NamedTuple):
    """VAR.compress: blobs[b] the self-describing byte string of image b, nbytes (B,) int64 their lengths, ideal_bits (B, S)
    float64: per scale sum log2(2^PB / F_token) of the coded tokens under the integer tables (0 for scales not coded)"""
    blobs: list
    nbytes: torch.Tensor
    ideal_bits: torch.Tensor
    patch_nums: tuple


class DecompressResult(NamedTuple):
    """VAR.decompress: tokens (B, L) int64 (-1 past the coded scales unless they were completed), images (B, 3, H, W) in [0, 1] or None,
    labels (B,) int64 from the blobs, scales: the index of the last coded scale"""
    tokens: torch.Tensor
    images: Optional[torch.Tensor]
    labels: torch.Tensor
    scales: int


CODEC_MAGIC, CODEC_VERSION = b'VARC', 1
_CODEC_HEAD = '<4sHBBIHHiIdQI'          # magic, version, PB, S, V, scales coded, 0, label, 0, cfg, token hash, word count; then S x uint16 patch_nums


def codec_token_hash(tok: np.ndarray) -> int:
    """64-bit hash of a token sequence: sum_i (tok_i + 1) * M^(n - i) mod 2^64, M = 0x9E3779B97F4A7C15 (odd: every position counts)"""
    tok = np.asarray(tok, np.int64).astype(np.uint64) + np.uint64(1)
    with np.errstate(over='ignore'):
        pw = np.cumprod(np.full(tok.shape[0], 0x9E3779B97F4A7C15, np.uint64))[::-1]
        return int((tok * pw).sum(dtype=np.uint64))


def codec_pack(words: np.ndarray, label: int, cfg: float, V: int, patch_nums, coded: int, tok_hash: int, pb: int) -> bytes:
    import struct
    head = struct.pack(_CODEC_HEAD, CODEC_MAGIC, CODEC_VERSION, pb, len(patch_nums), V, coded, 0, int(label), 0, float(cfg), tok_hash, int(words.shape[0]))
    return head + struct.pack(f'<{len(patch_nums)}H', *patch_nums) + np.asarray(words, '<u4').tobytes()


def codec_unpack(blob: bytes) -> dict:
    """the header and words of one blob; ValueError on anything that is no blob of this version"""
    import struct
    n0 = struct.calcsize(_CODEC_HEAD)
    if not isinstance(blob, (bytes, bytearray, memoryview)) or len(blob) < n0:
        raise ValueError('decompress: a blob is a bytes object made by VAR.compress')
    blob = bytes(blob)
    magic, ver, pb, S, V, coded, _, label, _, cfg, th, nw = struct.unpack_from(_CODEC_HEAD, blob)
    if magic != CODEC_MAGIC or ver != CODEC_VERSION:
        raise ValueError(f'decompress: not a VAR token blob of version {CODEC_VERSION}')
    if len(blob) != n0 + 2 * S + 4 * nw:
        raise ValueError(f'decompress: the blob holds {len(blob)} bytes, its header announces {n0 + 2 * S + 4 * nw}')
    pns = struct.unpack_from(f'<{S}H', blob, n0)
    return dict(pb=pb, V=V, coded=coded, label=label, cfg=cfg, hash=th, patch_nums=tuple(pns), words=np.frombuffer(blob, '<u4', nw, n0 + 2 * S))


class SharedAdaLin(nn.Linear):
    def forward(self, cond_BD):
        return super().forward(cond_BD).view(-1, 1, 6, self.weight.shape[0] // 6)


class VAR(nn.Module):
    def __init__(self, vae_local: VQVAE, num_classes=1000, depth=16, embed_dim=1024, num_heads=16, mlp_ratio=4., drop_rate=0.,
                 attn_drop_rate=0., drop_path_rate=0., norm_eps=1e-6, shared_aln=False, cond_drop_rate=0.1, attn_l2_norm=False,
                 patch_nums=(1, 2, 3, 4, 5, 6, 8, 10, 13, 16), flash_if_available=True, fused_if_available=True):
        super().__init__()
        assert embed_dim % num_heads == 0
        self.Cvae, self.V = vae_local.Cvae, vae_local.vocab_size
        self.depth, self.C, self.D, self.num_heads = depth, embed_dim, embed_dim, num_heads
        self.cond_drop_rate, self.prog_si, self.norm_eps, self.shared_aln = cond_drop_rate, -1, norm_eps, shared_aln
        self.patch_nums: Tuple[int] = tuple(patch_nums)
        sizes = [pn * pn for pn in self.patch_nums]
        self.L, self.first_l = sum(sizes), sizes[0]
        ends = torch.tensor(sizes).cumsum(0).tolist()
        self.begin_ends = list(zip([0] + ends[:-1], ends))
        self.num_stages_minus_1 = len(self.patch_nums) - 1
        self.rng = torch.Generator(device=dist.get_device())

        self.vae_proxy: Tuple[VQVAE] = (vae_local,)                          # tuples: the VAE is not a sub-module (not in our state-dict)
        self.vae_quant_proxy: Tuple[VectorQuantizer2] = (vae_local.quantize,)
        self.word_embed = nn.Linear(self.Cvae, self.C)

        std = math.sqrt(1 / self.C / 3)
        tn = lambda *shape: nn.init.trunc_normal_(torch.empty(*shape), mean=0, std=std)
        self.num_classes = num_classes
        self.uniform_prob = torch.full((1, num_classes), fill_value=1.0 / num_classes, dtype=torch.float32, device=dist.get_device())
        self.class_emb = nn.Embedding(num_classes + 1, self.C)
        nn.init.trunc_normal_(self.class_emb.weight.data, mean=0, std=std)
        self.pos_start = nn.Parameter(tn(1, self.first_l, self.C))
        self.pos_1LC = nn.Parameter(torch.cat([tn(1, n, self.C) for n in sizes], dim=1))
        self.lvl_embed = nn.Embedding(len(self.patch_nums), self.C)
        nn.init.trunc_normal_(self.lvl_embed.weight.data, mean=0, std=std)

        self.shared_ada_lin = nn.Sequential(nn.SiLU(inplace=False), SharedAdaLin(self.D, 6 * self.C)) if shared_aln else nn.Identity()
        norm_layer = partial(nn.LayerNorm, eps=norm_eps)
        self.drop_path_rate = drop_path_rate
        dpr = torch.linspace(0, drop_path_rate, depth).tolist()
        self.blocks = nn.ModuleList(
            AdaLNSelfAttn(cond_dim=self.D, shared_aln=shared_aln, block_idx=i, embed_dim=self.C, norm_layer=norm_layer, num_heads=num_heads,
                          mlp_ratio=mlp_ratio, drop=drop_rate, attn_drop=attn_drop_rate, drop_path=dpr[i], last_drop_p=0 if i == 0 else dpr[i - 1],
                          attn_l2_norm=attn_l2_norm, flash_if_available=flash_if_available, fused_if_available=fused_if_available)
            for i in range(depth))
        self.using_fused_add_norm_fn = False
        print(f'\n[constructor]  ==== MI355X HIP sampling path (var_amd); VAR config: embed_dim={embed_dim}, num_heads={num_heads}, depth={depth}, '
              f'mlp_ratio={mlp_ratio}, drop_path_rate={drop_path_rate:g}, patch_nums={self.patch_nums} ====\n', flush=True)

        lvl = torch.cat([torch.full((n,), i) for i, n in enumerate(sizes)]).view(1, self.L, 1)
        self.register_buffer('lvl_1L', lvl.transpose(1, 2)[:, 0].contiguous())
        self.register_buffer('attn_bias_for_masking', torch.where(lvl >= lvl.transpose(1, 2), 0., -torch.inf).reshape(1, 1, self.L, self.L).contiguous())

        self.head_nm = AdaLNBeforeHead(self.C, self.D, norm_layer=norm_layer)
        self.head = nn.Linear(self.C, self.V)
        self._engine = None

    # ---- HIP sampling path ------------------------------------------------------------------------------------------
    def engine(self):
        if self._engine is None:
            from ..engine import SamplingEngine
            self._engine = SamplingEngine(self)
        return self._engine

    def set_hip_precision(self, precision: str = 'f32'):
        """'f32' (default: tokens bit-identical to the CPU oracle, pixels within 1e-3 of the reference), 'f16' / 'bf16': 16-bit weights / GEMM
        operands / KV cache with fp32 accumulation — the arithmetic the reference's harness requests through
        torch.autocast('cuda', dtype=torch.float16) (demo_sample.py:66-68) — selected explicitly (an enclosing autocast context does not
        change the result of any of the three), or 'auto': every call follows the caller's autocast state the way the reference does
        (basic_var.py:97 branches on the dtype autocast hands it): inside torch.autocast('cuda', dtype=float16 | bfloat16) the call runs the
        matching 16-bit mode, outside it (or with enabled=False) f32.  With 'auto' demo_sample.py runs its fp16 path unchanged.
        The environment variable VARHIP_FOLLOW_AUTOCAST=1 makes 'auto' the initial policy of every new engine (default: 'f32')."""
        self.engine().set_precision(precision)
        return self

    @torch.no_grad()
    def autoregressive_infer_cfg(self, B: int, label_B: Optional[Union[int, torch.LongTensor]], g_seed: Optional[int] = None, cfg=1.5,
                                 top_k=0, top_p=0.0, more_smooth=False) -> torch.Tensor:
        """Sample B images; returns (B, 3, H, W) in [0, 1].  Same arguments and RNG consumption as the reference
        (var.py:126-190): `g_seed` seeds self.rng, one Exp(1) fill of shape (B*l, V) is drawn per scale."""
        self._hip_only('autoregressive_infer_cfg')
        rng, lab = self._rng_and_labels(B, label_B, g_seed, negative_is_uncond=True, seeded_draw=True)
        return self.engine().sample(B, lab, rng, cfg, top_k, top_p, more_smooth=bool(more_smooth))

    def _hip_only(self, name: str, loop: str = 'sampling loop', how: str = '; move the model to a CUDA/ROCm device (there is no CPU fallback by design)'):
        """the model's device; a model off the GPU is refused: the sampling calls have no PyTorch implementation"""
        dev = self.lvl_1L.device
        if dev.type != 'cuda':
            raise RuntimeError(f'VAR.{name}: this build runs the {loop} on MI355X HIP kernels only{how}')
        return dev

    def _rng_and_labels(self, B, label_B, g_seed, *, negative_is_uncond: bool, seeded_draw: bool, name: str = 'label_B'):
        """g_seed and label_B of the reference-style sampling calls -> (self.rng seeded with g_seed, or None; (B,) int64 labels on the model's
        device).  negative_is_uncond: an int label below 0 means num_classes.  seeded_draw: labels for label_B=None are drawn from that rng
        (autoregressive_infer_cfg*); otherwise from torch's global generator, as the reference's inpainting and smooth_sampling do."""
        dev = self.lvl_1L.device
        if g_seed is None: rng = None
        else: self.rng.manual_seed(g_seed); rng = self.rng
        if label_B is None:
            label_B = torch.multinomial(self.uniform_prob, num_samples=B, replacement=True, generator=rng if seeded_draw else None).reshape(B)
        elif isinstance(label_B, bool):
            raise ValueError(f'{name} must be None, an int or {B} integer class ids')
        elif A.is_int(label_B):
            label_B = torch.full((B,), fill_value=self.num_classes if negative_is_uncond and label_B < 0 else int(label_B), device=dev)
        return rng, label_B.to(dev).long()

    def _record(self, img, tok, st) -> SampleRecord:
        return SampleRecord(img, tok, st['logp_cond'], st['logp_guided'], st['logp_drawn'], st['entropy'], st['kept'], self.patch_nums)

    @torch.no_grad()
    def autoregressive_infer_cfg_scored(self, B: int, label_B: Optional[Union[int, torch.LongTensor]], g_seed: Optional[int] = None, cfg=1.5,
                                        top_k=0, top_p=0.0, more_smooth=False, decode=True) -> SampleRecord:
        """autoregressive_infer_cfg that also returns what the sampler knew about every token it drew: a SampleRecord with the tokens, their
        log-probability under the conditional, the guided and the filtered (actually drawn-from) distribution, the guided entropy and the
        number of codes top-k / top-p kept.  Same argument handling and RNG consumption as autoregressive_infer_cfg; images and tokens are
        bit-identical to that call with the same arguments.  The numbers come from one reduction per scale behind the sampler
        (varhip_sample_stats_f32) on logits that are in memory anyway: no second transformer pass, as token_log_likelihood on the tokens
        would need.  decode=False skips the decoder (images is None)."""
        dev = self._hip_only('autoregressive_infer_cfg_scored')
        rng, lab = self._rng_and_labels(B, label_B, g_seed, negative_is_uncond=True, seeded_draw=True)
        tok = torch.empty(B, self.L, dtype=torch.int64, device=dev)
        st = {}
        img = self.engine().sample(B, lab, rng, cfg, top_k, top_p, more_smooth=bool(more_smooth), tokens_out=tok,
                                   decode=bool(decode), stats=st)
        return self._record(img if decode else None, tok, st)

    @torch.no_grad()
    def autoregressive_infer_cfg_per_image_scored(self, label_B, g_seeds, cfg=1.5, top_k=0, top_p=0.0, more_smooth=False, decode=True) -> SampleRecord:
        """autoregressive_infer_cfg_per_image (own seed, cfg, top_k, top_p per image; the project's counter-based noise stream) with the
        SampleRecord of autoregressive_infer_cfg_scored.  The tokens and every per-token field of image b depend on that request alone, not on
        what it is batched with (pixels: as for the per-image call, the decoder's kernel choice follows the batch).  HIP path only."""
        dev = self._hip_only('autoregressive_infer_cfg_per_image_scored')
        lab, seeds, cfgs, ks, ps = self._per_image_args(label_B, g_seeds, cfg, top_k, top_p)
        tok = torch.empty(lab.numel(), self.L, dtype=torch.int64, device=dev)
        st = {}
        img = self.engine().sample_per_image(lab.to(dev).long(), seeds, cfgs, ks, ps, more_smooth=bool(more_smooth), tokens_out=tok,
                                             decode=bool(decode), stats=st)
        return self._record(img if decode else None, tok, st)

    @torch.no_grad()
    def sample_composed(self, labels, weights, g_seeds, cfg=1.5, top_k=0, top_p=0.0, max_rows: int = 128, decode=True) -> ComposedRecord:
        """Sample with K classes per image guiding one token stream: hybrids (weights 0.5 / 0.5), a negative class (a weight below 0), and a
        schedule over the scales (class A on the coarse scales, class B on the fine ones).
          labels    (B, K) integer class ids in [0, num_classes], 1 <= K <= 8
          weights   (B, K), the same on every scale, or (S, B, K), one set per scale; finite, any sign, zero allowed
          g_seeds, cfg, top_k, top_p: per image as in autoregressive_infer_cfg_per_image (a scalar for all or B values; the same Philox stream)
        The sampler of image b at scale s draws from the row (t = cfg_b * s / (S - 1), W = sum_k w_k)
            x = (1 + t) * sum_k w_k c_k - (t + (1 + t)(W - 1)) u     =  u + (1 + t) * sum_k w_k (c_k - u)
        with c_k the logits under class k and u the unconditional ones: K = 1, w = 1 is autoregressive_infer_cfg_per_image_scored bit for bit.
        The K + 1 coefficients are formed on the host in float64 and rounded once to fp32 (ComposedRecord.coef), the kernel adds the products
        in class order, each operation rounded to fp32 (varhip_mix_sample_rows_f32).  The images run in passes of at most max_rows transformer
        rows, K + 1 per image; a request's tokens and record do not depend on the pass or the batch it is in.  decode=False skips the decoder.
        HIP path only (a CUDA / ROCm model in eval mode); no more_smooth, no edit mask (SamplingEngine.sample_composed)."""
        lab, w, seeds, cfgs, ks, ps = A.compose_args(self.V, self.num_classes, len(self.patch_nums), labels, weights, g_seeds, cfg, top_k, top_p, max_rows)
        dev = self._hip_only('sample_composed')
        if self.training or self.prog_si >= 0:
            raise RuntimeError('VAR.sample_composed: this build runs the sampling loop on MI355X HIP kernels only; put the model in eval mode with prog_si < 0')
        from ..engine import compose_tables
        coef = compose_tables(cfgs, w, len(self.patch_nums))
        r = self.engine().sample_composed(lab.to(dev), coef, seeds, cfgs, ks, ps, int(max_rows), bool(decode))
        return ComposedRecord(r['images'], r['tokens'], r['logp_class'], r['logp_guided'], r['logp_drawn'], r['entropy'], r['kept'], coef, lab, self.patch_nums)

    @torch.no_grad()
    def sample_controlled(self, label_B, g_seeds, cfg=1.5, top_k=0, top_p=0.0, *, temperature=1.0, min_p=0.0, logit_bias=None, cfg_ramp=True,
                          decode=True) -> SampleRecord:
        """autoregressive_infer_cfg_per_image_scored with the sampler's full set of controls, each per image and per scale.
          label_B, g_seeds   as in autoregressive_infer_cfg_per_image: (B,) class ids, (B,) seeds in [0, 2^63) (the same Philox stream)
          cfg, top_k, top_p, temperature, min_p   each a scalar, (B,) values per image, or (S, B) per scale and image; a B axis of size 1
                             broadcasts, so (S, 1) is a pure per-scale schedule.  temperature finite and > 0 (for the limit 0 use top_k=1),
                             min_p in [0, 1], top_k in [0, V], top_p in [0, 1]
          logit_bias         None, (V,) for every request, (B, V) or (S, B, V) (a size-1 B broadcasts): added to the guided logits; -inf bans a
                             code; no NaN, no +inf, and not every code of a row banned
          cfg_ramp           True: t = cfg * s / (S - 1), the reference's ramp, as every other call; False: t = cfg, the schedule is the caller's
        Per token row, in this order: x = (1 + t) * cond - t * uncond;  x += bias;  x /= temperature;  top-k;  min-p: with p_max the largest
        probability of what top-k left, codes with p_v < min_p * p_max go (exp(x_v - max x) < min_p, compared in fp32);  top-p;  the draw.  A
        stage whose knob is neutral (no bias, temperature 1, top_k 0, min_p 0, top_p 0) does not run: with every control at its default
        the record and the images are autoregressive_infer_cfg_per_image_scored's bit for bit.
        The record (SampleRecord): logp_cond and logp_guided keep their meaning — they are computed before bias and temperature, so with
        cfg_ramp=True and a cfg that is not scheduled logp_guided is bit-equal in f32 to token_log_likelihood of the drawn tokens at that
        cfg; entropy is the guided row's.  logp_drawn and kept describe the biased, tempered and filtered row the token was drawn from.
        A request's tokens and record depend on its own label, seed and controls only, not on what it is batched with — except that a
        logit_bias given as (V,) is by definition part of every request of the call.  On the HIP path (a CUDA / ROCm model in eval mode,
        prog_si < 0; f32, f16 and bf16) the sampler is varhip_ctl_sample_rows_f32 (SamplingEngine.sample_controlled).
        Elsewhere (a CPU model, train mode, prog_si >= 0) the loop runs in PyTorch, request by request, with the stages in torch fp32 and the
        host Philox fill; the per-image scored call has no statistics there, and this one has none either: images and tokens are
        returned, the five per-token fields are None.  No more_smooth."""
        lab, seeds = self._per_image_args(label_B, g_seeds, 0.0, 0, 0.0)[:2]
        B, dev = lab.numel(), self.lvl_1L.device
        from ..engine import control_tables
        tab = control_tables(cfg, top_k, top_p, temperature, min_p, logit_bias, len(self.patch_nums), self.V, B, bool(cfg_ramp))
        lab = lab.to(dev).long()
        if dev.type == 'cuda' and not self.training and self.prog_si < 0:
            tok = torch.empty(B, self.L, dtype=torch.int64, device=dev)
            st = {}
            img = self.engine().sample_controlled(lab, seeds, tab, tokens_out=tok, decode=bool(decode), stats=st)
            return self._record(img if decode else None, tok, st)
        self.engine()._check_labels(lab)
        img, tok = self._per_image_torch(lab, seeds, None, None, None, False, ctl=tab)
        return SampleRecord(img if decode else None, tok, None, None, None, None, None, self.patch_nums)

    def _counterfactual_begin(self, name: str):
        dev = self._hip_only(name)
        if self.training or self.prog_si >= 0:
            raise RuntimeError(f'VAR.{name}: this build runs the sampling loop on MI355X HIP kernels only; put the model in eval mode with prog_si < 0')
        return dev

    @torch.no_grad()
    def abduct_noise(self, gt_tokens, label_B, g_seeds, cfg=1.5, first_scale=0, max_images=8) -> NoiseRecord:
        """The noise under which the model would have produced these tokens: for every token of scales >= first_scale, a draw from the law
        of the sampler's Exp(1) noise given that the unfiltered guided sampler (label_B, cfg, no top-k / top-p) returned it — the Gumbel-max
        posterior in the exponential-race form the sampler uses.  Replayed under the same label and cfg it gives
        the tokens back bit for bit; replayed under another label it gives the coupled sample (VAR.counterfactual).
          gt_tokens  (B, L) integer token ids in [0, V), e.g. vae.img_to_idxBl's, concatenated
          label_B    (B,) class ids;  g_seeds (B,) integers in [0, 2^63): the fresh values come from the per-image Philox stream of seed b
                     (draws 2 and 3: the record of a request does not depend on what it is batched with, self.rng is not touched)
          cfg        a scalar or B values;  first_scale in [0, S];  max_images: images per pass
        One teacher-forced walk (no decode) with varhip_exp1_posterior_f32 behind each head; f32, f16 and bf16.  The record costs
        L * V * 4 bytes per image (11.1 MB at 256 px, 36.7 MB at 512 px).  HIP path only."""
        a = A.counterfactual_args(self.V, self.L, len(self.patch_nums), self.num_classes, gt_tokens, label_B, None, g_seeds, cfg, None, 0, 0.0,
                                  first_scale, max_images)
        dev = self._counterfactual_begin('abduct_noise')
        gt, lab, B, m = a['gt'].to(dev).long(), a['lab_src'].to(dev).long(), a['gt'].shape[0], a['max_images']
        eng = self.engine()
        parts = [eng.abduct(gt[b0:b0 + m], lab[b0:b0 + m].contiguous(), a['seeds'][b0:b0 + m], a['cfg'][b0:b0 + m], a['first']) for b0 in range(0, B, m)]
        cat = lambda key: parts[0][key] if len(parts) == 1 else torch.cat([p[key] for p in parts])
        return NoiseRecord(cat('noise'), cat('logp'), cat('flags').ne(0), a['cfg'], a['first'], parts[0]['precision'], parts[0]['sig'])

    @torch.no_grad()
    def counterfactual(self, gt_tokens, label_src, label_dst, g_seeds, cfg=1.5, cfg_dst=None, top_k=0, top_p=0.0, first_scale=0, noise=None,
                       decode=True, max_images=8) -> CounterfactualResult:
        """Re-sample given images under another class with their own noise: abduct_noise(gt_tokens, label_src, g_seeds, cfg, first_scale), then
        the per-image sampler replays that noise under label_dst — what the model would have drawn, had the class been another, everything
        else being equal.  Tokens the target distribution still prefers under that noise stay; the others move.
          label_dst  (B,) or (B, K): K replays of one abduction;  cfg_dst (default: cfg), top_k, top_p: the TARGET side's, per image
          first_scale  scales below it are kept as given (forced through the kept-scale route), the rest is replayed
          noise      a NoiseRecord of an earlier call on the same tokens, label_src, seeds and cfg: no second abduction.  A record made in
                     another precision, under other weights or with a larger first_scale raises ValueError
        With label_dst == label_src, cfg_dst == cfg and no filter the result is gt_tokens bit for bit wherever `unreachable` is false.
        Source-side filters are not offered (a token outside a filter has no noise that explains it); no more_smooth.  A request's result
        does not depend on its batch, on K or on max_images (which chunks both phases); self.rng is neither read nor advanced.  HIP path only
        (SamplingEngine.abduct / .counterfactual)."""
        S = len(self.patch_nums)
        a = A.counterfactual_args(self.V, self.L, S, self.num_classes, gt_tokens, label_src, label_dst, g_seeds, cfg, cfg_dst, top_k, top_p,
                                  first_scale, max_images)
        dev = self._counterfactual_begin('counterfactual')
        eng = self.engine()
        gt, B, K, m, first = a['gt'].to(dev).long().contiguous(), a['gt'].shape[0], a['lab_dst'].shape[1], a['max_images'], a['first']
        if noise is None:
            noise = self.abduct_noise(gt, a['lab_src'], a['seeds'], a['cfg'], first, m)
        else:
            if not isinstance(noise, NoiseRecord) or tuple(noise.noise.shape) != (B, self.L, self.V) or noise.noise.device != gt.device:
                raise ValueError(f'noise must be a NoiseRecord of these {B} images on the model\'s device')
            prec = eng.resolve_precision()
            eng.refresh()
            if noise.precision != prec:
                raise ValueError(f'the NoiseRecord was made in {noise.precision}, this call runs in {prec}: the logits differ, the noise explains nothing')
            if noise._sig != eng._sig:
                raise ValueError('the NoiseRecord was made under other weights')
            if noise.first_scale > first:
                raise ValueError(f'the NoiseRecord starts at scale {noise.first_scale}: it holds no noise for first_scale = {first}')
        R = B * K
        rows = torch.arange(B, device=dev).repeat_interleave(K)
        lab = a['lab_dst'].to(dev).long().reshape(-1).contiguous()
        gt_rows = gt.index_select(0, rows)
        tok = torch.empty(R, self.L, dtype=torch.int64, device=dev)
        st = {key: torch.zeros(R, self.L, dtype=torch.int32, device=dev) if key == 'kept' else torch.full((R, self.L), float('nan'), device=dev)
              for key in SampleRecord.FIELDS}
        imgs = []
        for c0 in range(0, R, m):
            c1 = min(c0 + m, R)
            imgs.append(eng.counterfactual(noise.noise, rows[c0:c1], gt_rows[c0:c1], lab[c0:c1], a['cfg_dst'][c0:c1], a['top_k'][c0:c1], a['top_p'][c0:c1],
                                           first, tok[c0:c1], {key: v[c0:c1] for key, v in st.items()}, bool(decode)))
        img = torch.cat(imgs) if decode else None
        changed = tok.ne(gt_rows)
        per_scale = torch.stack([changed[:, b0:e0].any(1) for b0, e0 in self.begin_ends], dim=1)                # (R, S)
        fcs = torch.where(per_scale.any(1), per_scale.to(torch.int64).argmax(1), torch.full((R,), S, dtype=torch.int64, device=dev))
        return CounterfactualResult(None if img is None else img.view(B, K, *img.shape[1:]), tok.view(B, K, self.L), changed.view(B, K, self.L),
                                    fcs.view(B, K), noise.logp_src, noise.unreachable, self._record(img, tok, st), noise, self.patch_nums)

    @torch.no_grad()
    def sample_best_of(self, label_B, g_seeds, n: Optional[int] = None, by: str = 'logp_cond', cfg=1.5, top_k=0, top_p=0.0, max_images: int = 64):
        """Best-of-n sampling: n candidates per image, ranked by their own likelihood, only the winners decoded.
          label_B   (B,) integer class ids;  g_seeds (B, n) integers in [0, 2^63), one seed per candidate;  n: optional, must equal g_seeds' width
          by        'logp_cond' | 'logp_guided' | 'logp_drawn': the SampleRecord field whose sum over the L tokens ranks the candidates
          cfg, top_k, top_p: a scalar, or B values (one per image, shared by its candidates)
        -> (images (B, 3, H, W), winners: the SampleRecord of the B chosen candidates, totals (B, n) float64, choice (B,) int64).
        The B * n candidates run through the per-image path with decode=False in chunks of at most max_images, so a candidate is exactly the
        request autoregressive_infer_cfg_per_image_scored(label, seed, ...) and does not depend on the chunking; each one's f_hat (Cvae * P * P
        floats) is kept.  totals[b, c] is the float64 sum of the field in token order; varhip_class_select_f32 picks per image the highest total
        on the device (NaN below everything, ties to the lower index), and only those B f_hat maps are gathered and decoded: the decoder is
        the most expensive single stage of a call and runs for 1 of n candidates."""
        dev = self._hip_only('sample_best_of')
        B, n, lab, seeds, cfgs, ks, ps, sd = A.candidate_args(self.V, BEST_OF_FIELDS, label_B, g_seeds, n, by, cfg, top_k, top_p, max_images)
        rec, f_hat, totals, choice = self.engine().sample_best_of(lab.to(dev).long(), seeds, cfgs, ks, ps, n, by, int(max_images))
        img = self.engine().decode_f_hat(f_hat)
        return img, self._record(img, rec.pop('tokens'), rec), totals, choice

    @torch.no_grad()
    def sample_best_of_pruned(self, label_B, g_seeds, keep, n: Optional[int] = None, by: str = 'logp_cond', cfg=1.5, top_k=0, top_p=0.0,
                              max_images: int = 64, decode: bool = True) -> BestOfResult:
        """Best-of-n sampling that drops candidates by scale -> BestOfResult(images, winners, totals, depth, choice, tokens).
        label_B, g_seeds (B, n), n, by, cfg, top_k, top_p and max_images mean what they mean in sample_best_of.  keep: None / {} (no pruning: the
        result of sample_best_of) or {scale: m}, 0 <= scale < S-1, integer m >= 1, as in classify: behind that scale each image keeps its m best
        surviving candidates by the running total of `by` (an m at or above the survivor count drops nothing), and the others are sampled no
        further: a dropped candidate costs no transformer time past its scale, the survivors go on in a smaller batch.  The rule at every
        boundary and for choice is sample_best_of's: the float64 total in token order, highest first, NaN below everything, ties to the lower
        index.  Every candidate, through its depth, is bit for bit the request autoregressive_infer_cfg_per_image_scored(label, seed, ...) run
        alone, whatever it was batched with and whatever max_images is; self.rng is neither read nor advanced.
          totals (B, n) float64: each candidate's running total at its depth;  depth (B, n) int64: the last scale it was sampled through
          choice (B,) int64: the best full-depth candidate;  tokens (B, n, L) int64: every candidate's tokens, -1 past its depth
          winners: the SampleRecord of the B chosen candidates;  images: their decoded images (None with decode=False)
        Chunks hold max_images // n whole images (n > max_images raises ValueError).  Whether an early total predicts the final rank depends on
        the weights: that trade-off is the caller's, as with classify's keep.  HIP path only (SamplingEngine.sample_best_of_pruned, DESIGN.md
        section 30)."""
        dev = self._hip_only('sample_best_of_pruned')
        B, n, lab, seeds, cfgs, ks, ps, sd = A.candidate_args(self.V, BEST_OF_FIELDS, label_B, g_seeds, n, by, cfg, top_k, top_p, max_images, 'candidates')
        schedule = normalize_keep(keep, len(self.patch_nums), n)
        eng = self.engine()
        rec, f_hat, totals, depth, choice = eng.sample_best_of_pruned(lab.to(dev).long(), seeds, cfgs, ks, ps, n, by, schedule, int(max_images))
        img = eng.decode_f_hat(f_hat) if decode else None
        pick = choice.view(B, 1, 1).expand(B, 1, self.L)
        win = {key: v.gather(1, pick)[:, 0] for key, v in rec.items()}
        return BestOfResult(img, self._record(img, win.pop('tokens'), win), totals, depth, choice, rec['tokens'])

    @torch.no_grad()
    def sample_smc(self, label_B, g_seeds, resample=(4, 6), n: Optional[int] = None, by: str = 'logp_cond', beta: float = 1.0, ess=0.5,
                   cfg=1.5, top_k=0, top_p=0.0, max_images: int = 64, decode: bool = True, resample_seeds=None) -> SMCResult:
        """n particles per image with resampling at scale boundaries (a particle filter over the scales) -> SMCResult.
        label_B, g_seeds (B, n), n, by, cfg, top_k, top_p and max_images mean what they mean in sample_best_of_pruned.
          resample   boundary scales, ascending, unique, below the last scale (an empty sequence: no boundary)
          beta       the weight's inverse temperature (a finite float)
          ess        a float in (0, 1]: an image resamples behind a boundary when its effective sample size is below ess * n; None: always
          resample_seeds  (B,) integers in [0, 2^63), the key of each image's resampling uniform; default g_seeds[:, 0]
        What the particles approximate: every token is drawn from the filtered, guided distribution (cfg, top_k, top_p), which is the proposal;
        behind a stage a particle's incremental weight is exp(beta * sum of `by` over the stage's tokens).  Behind a boundary scale the weak
        particles die and the strong ones are copied into their slots (systematic resampling, one uniform per (image, boundary); survivors
        stay in their own slots; the weights restart at 1), so the call ends with n images per label that share good coarse scales and differ
        in the fine ones: slot c keeps its own seed g_seeds[b][c], so a copy diverges from its parent from the next scale on, its noise there
        keyed by (slot seed, scale).  The weighted particles target the proposal tilted by exp(beta * sum `by`); beta = 0 gives equal weights
        (ess == n: no threshold resamples), a large beta with ess=None tends to "keep the best and refill".  Without a resampling event the
        particles are bit for bit autoregressive_infer_cfg_per_image_scored on the same labels and seeds, and at beta = 1 log_weights are
        sample_best_of's totals.  An image's result depends on its own label, seeds and parameters only, not on what it is batched with or on
        max_images (pixels: as for the per-image call, the decoder's kernel choice follows its batch); self.rng is neither read nor advanced.  The K and V caches are resampled in place (varhip_kv_resample: only the rows that
        died are copied), so the call needs no second cache set and the late scales run the full batch.  Chunks hold max_images // n whole
        images (n > max_images raises ValueError).  HIP path only, no more_smooth (SamplingEngine.sample_smc)."""
        dev = self._hip_only('sample_smc')
        if ess is not None:
            A.real(ess, f'ess must be None (always resample) or a float in (0, 1], got {ess!r}', lambda v: 0.0 < v <= 1.0)
        A.real(beta, f'beta must be a finite float, got {beta!r}')
        bounds = normalize_resample(resample, len(self.patch_nums))
        B, n, lab, seeds, cfgs, ks, ps, sd = A.candidate_args(self.V, BEST_OF_FIELDS, label_B, g_seeds, n, by, cfg, top_k, top_p, max_images, 'particles')
        lab0 = lab[::n]                                        # (lab holds each image's label n times)
        rs = [r[0] for r in sd] if resample_seeds is None else self._per_image_args(lab0, resample_seeds, 0.0, 0, 0.0)[1]
        eng = self.engine()
        res = eng.sample_smc(lab.to(dev).long(), seeds, cfgs, ks, ps, n, by, bounds, float(beta), -1.0 if ess is None else float(ess), rs, int(max_images))
        img = None
        if decode:
            f_hat = res['f_hat']
            img = torch.cat([eng.decode_f_hat(f_hat[c0:c0 + int(max_images)]) for c0 in range(0, B * n, int(max_images))])
            img = img.view(B, n, *img.shape[1:])
        st = {key: res[key] for key in SampleRecord.FIELDS}
        return SMCResult(img, self._record(None if img is None else img.view(B * n, *img.shape[2:]), res['tokens'], st), res['log_weights'],
                         res['ancestors'], res['resampled'], res['ess'], res['log_weights_seen'], tuple(self.patch_nums))

    @torch.no_grad()
    def autoregressive_infer_cfg_per_image(self, label_B, g_seeds, cfg=1.5, top_k=0, top_p=0.0, more_smooth=False, return_tokens=False):
        """Sample a batch of unrelated requests: image b is drawn with its own seed g_seeds[b] and its own cfg / top_k / top_p (each a scalar
        for all, or B values).  Returns (B, 3, H, W) fp32 in [0, 1]; with return_tokens=True also the (B, L) int64 tokens.
        Guarantee: the tokens of a request depend on (label, seed, cfg, top_k, top_p, more_smooth) and the weights only — not on the batch
        size, the request's position in the batch or its neighbours.  The noise is the project's own counter-based stream (Philox4x32-10
        keyed by the seed, counter (column / 4, row, scale, draw): include/var_hip.h, varhip_exp1_philox_f32), NOT torch's: the images
        differ from autoregressive_infer_cfg(g_seed=...) with the same numbers, and self.rng is neither read nor advanced.
          label_B   (B,) integer tensor or list, labels in [0, num_classes] (num_classes = unconditional)
          g_seeds   (B,) integers in [0, 2^63)
        more_smooth is one bool for the batch.  Precision follows set_hip_precision / 'auto' as the plain call does.  On the HIP path (a CUDA /
        ROCm model in eval mode, prog_si < 0) the loop is SamplingEngine.sample_per_image; elsewhere (a CPU model, train mode, prog_si >= 0)
        the same stream comes from the library's host twin and the loop runs in PyTorch, image by image."""
        lab, seeds, cfgs, ks, ps = self._per_image_args(label_B, g_seeds, cfg, top_k, top_p)
        B = lab.numel()
        dev = self.lvl_1L.device
        lab = lab.to(dev).long()
        if dev.type == 'cuda' and not self.training and self.prog_si < 0:
            tok = torch.empty(B, self.L, dtype=torch.int64, device=dev) if return_tokens else None
            img = self.engine().sample_per_image(lab, seeds, cfgs, ks, ps, more_smooth=bool(more_smooth), tokens_out=tok)
            return (img, tok) if return_tokens else img
        self.engine()._check_labels(lab)
        img, tok = self._per_image_torch(lab, seeds, cfgs, ks, ps, bool(more_smooth))
        return (img, tok) if return_tokens else img

    def _per_image_args(self, label_B, g_seeds, cfg, top_k, top_p):
        """the argument handling of the per-image calls -> (labels (B,) integer tensor, seeds, cfgs, top_ks, top_ps: lists of B values)"""
        return A.sample_args(self.V, label_B, g_seeds, cfg, top_k, top_p)

    def _per_image_torch(self, lab, seeds, cfgs, ks, ps, more_smooth: bool, ctl: Optional[dict] = None):
        """the PyTorch side of autoregressive_infer_cfg_per_image (reference var.py:126-190, one request at a time): the Exp(1) fills are
        the host twin's (varhip_exp1_philox_host_f32), the sampler is helpers.py:6-19 with the multinomial written as argmax(p / noise).
        ctl: control_tables' result (sample_controlled; cfgs, ks and ps are then not read): t, top_k and top_p come from the tables' entry of
        (scale, request), and bias, temperature and min-p run in torch fp32 where varhip_ctl_sample_rows_f32 runs them."""
        from .. import hip
        vae, quant = self.vae_proxy[0], self.vae_quant_proxy[0]
        dev, S, V = lab.device, len(self.patch_nums), self.V
        imgs, toks = [], []

        def fill(seed, l, si, draw):
            out = np.empty((l, V), np.float32)
            hip.call_host('exp1_philox_host_f32', np.asarray([seed], np.int64), 1, l, V, si, draw, out)
            return torch.from_numpy(out).to(dev)
        for b in range(lab.numel()):
            cond_BD = self.class_emb(torch.stack((lab[b], torch.full_like(lab[b], self.num_classes))))
            sos = cond_BD
            lvl_pos = self.lvl_embed(self.lvl_1L) + self.pos_1LC
            x = sos.unsqueeze(1).expand(2, self.first_l, -1) + self.pos_start.expand(2, self.first_l, -1) + lvl_pos[:, :self.first_l]
            f_hat = sos.new_zeros(1, self.Cvae, self.patch_nums[-1], self.patch_nums[-1])
            cond_or_gss = self.shared_ada_lin(cond_BD)
            for blk in self.blocks: blk.attn.kv_caching(True)
            cur, tok = 0, []
            try:
                for si, pn in enumerate(self.patch_nums):
                    l = pn * pn
                    ratio = si / self.num_stages_minus_1 if self.num_stages_minus_1 > 0 else 0.0
                    cur += l
                    for blk in self.blocks:
                        x = blk(x=x, cond_BD=cond_or_gss, attn_bias=None)
                    z = self.get_logits(x, cond_BD)
                    t, k, p = (cfgs[b] * ratio, ks[b], ps[b]) if ctl is None else (float(ctl['t'][si, b]), int(ctl['top_k'][si, b]), float(ctl['top_p'][si, b]))
                    z = (1 + t) * z[:1] - t * z[1:]
                    if ctl is not None and ctl['bias_row'][si, b] >= 0:
                        z = z + torch.from_numpy(ctl['bias'][ctl['bias_row'][si, b]]).to(dev)
                    if ctl is not None and ctl['tau'][si, b] != 1:
                        z = z / torch.full_like(z, float(ctl['tau'][si, b]))          # (a tensor divisor: a true fp32 division on every backend)
                    if k > 0:
                        z = z.masked_fill(z < z.topk(k, largest=True, sorted=False, dim=-1)[0].amin(dim=-1, keepdim=True), -torch.inf)
                    if ctl is not None and ctl['min_p'][si, b] > 0:
                        z = z.masked_fill((z - z.amax(dim=-1, keepdim=True)).exp() < float(ctl['min_p'][si, b]), -torch.inf)
                    if p > 0:
                        srt, order = z.sort(dim=-1, descending=False)
                        drop = srt.softmax(dim=-1).cumsum_(dim=-1) <= (1 - p)
                        drop[..., -1:] = False
                        z = z.masked_fill(drop.scatter(order.ndim - 1, order, drop), -torch.inf)
                    idx = (z.softmax(dim=-1)[0] / fill(seeds[b], l, si, 0)).argmax(dim=-1).view(1, l)
                    tok.append(idx)
                    if more_smooth:
                        gum_t = max(0.27 * (1 - ratio * 0.95), 0.005)
                        g = -fill(seeds[b], l, si, 1).log()
                        h = ((z[0] * (1 + ratio) + g) / gum_t).softmax(dim=-1) @ quant.embedding.weight
                        h = h.view(1, l, self.Cvae)
                    else:
                        h = quant.embedding(idx)
                    h = h.transpose(1, 2).reshape(1, self.Cvae, pn, pn)
                    f_hat, nxt = quant.get_next_autoregressive_input(si, S, f_hat, h)
                    if si != S - 1:
                        nxt = nxt.view(1, self.Cvae, -1).transpose(1, 2)
                        nl = self.patch_nums[si + 1] ** 2
                        x = (self.word_embed(nxt) + lvl_pos[:, cur:cur + nl]).repeat(2, 1, 1)
            finally:
                for blk in self.blocks: blk.attn.kv_caching(False)
            imgs.append(vae.fhat_to_img(f_hat).add_(1).mul_(0.5))
            toks.append(torch.cat(tok, dim=1))
        return torch.cat(imgs), torch.cat(toks)

    @torch.no_grad()
    def autoregressive_infer_cfg_with_mask(self, B: int, label_B: Optional[Union[int, torch.LongTensor]], g_seed: Optional[int] = None, cfg=1.5,
                                           top_k=0, top_p=0.0, more_smooth=False, input_img_tokens=None, edit_mask=None) -> torch.Tensor:
        """Zero-shot editing (in-painting, out-painting, class-conditional editing): the loop of demo_zero_shot_edit.ipynb (cell 2) as a
        method, on the HIP engine.  Returns (B, 3, H, W) in [0, 1].  Labels, g_seed and RNG consumption are those of autoregressive_infer_cfg:
        every scale draws its (B*l, V) Exp(1) fill (and with more_smooth its gumbel fill) whatever the mask keeps.
          input_img_tokens  the S per-scale (B, pn^2) token tensors of vae.img_to_idxBl, or their (B, L) concatenation.  A single row is
                            used for all B rows (an extension: the notebook's loop needs B rows; one image with B edits is the usual case)
          edit_mask         (h, w) or (B, h, w) (a leading 1 broadcasts), any real or bool dtype, h, w >= 1: 1 keeps the input token, 0
                            generates a new one.  Per scale keep = F.interpolate(mask, (pn, pn), 'bilinear', align_corners=False) > 0.5, and
                            scales with pn * pn <= 3 are kept whole; kept positions take codebook[input token] (with more_smooth too).
        Both None: exactly autoregressive_infer_cfg.  Only one of them, or a malformed one: ValueError (checked before the device).  A model
        off the GPU: RuntimeError (no CPU fallback)."""
        if (input_img_tokens is None) != (edit_mask is None):
            raise ValueError('input_img_tokens and edit_mask go together: give both (editing) or neither (plain sampling)')
        if edit_mask is None:
            return self.autoregressive_infer_cfg(B, label_B, g_seed=g_seed, cfg=cfg, top_k=top_k, top_p=top_p, more_smooth=more_smooth)
        if isinstance(B, bool) or not isinstance(B, int) or B < 1:
            raise ValueError('B must be an integer >= 1')
        tokens = self._edit_tokens(input_img_tokens, B)
        mask = self._edit_mask(edit_mask, B)
        if isinstance(label_B, torch.Tensor) and (label_B.dtype.is_floating_point or label_B.dtype == torch.bool or label_B.numel() != B):
            raise ValueError(f'label_B must be None, an int or {B} integer class ids')
        dev = self._hip_only('autoregressive_infer_cfg_with_mask', 'editing loop')
        rng, lab = self._rng_and_labels(B, label_B, g_seed, negative_is_uncond=True, seeded_draw=True)
        tokens = tokens.to(dev).expand(B, -1).contiguous()
        return self.engine().sample(B, lab.reshape(B), rng, cfg, top_k, top_p, more_smooth=bool(more_smooth),
                                    edit=dict(tokens=tokens, mask=mask.to(dev)))

    def _edit_tokens(self, toks, B: int) -> torch.Tensor:
        """input_img_tokens -> (1 or B, L) int64 (still on the caller's device), shape, dtype and range checked"""
        if isinstance(toks, (list, tuple)):
            if len(toks) != len(self.patch_nums) or not all(isinstance(t, torch.Tensor) for t in toks):
                raise ValueError(f'input_img_tokens must be a list of {len(self.patch_nums)} per-scale token tensors (vae.img_to_idxBl)')
            rows = toks[0].shape[0] if toks[0].dim() == 2 else -1
            for t, pn in zip(toks, self.patch_nums):
                if t.dim() != 2 or t.shape[0] != rows or t.shape[1] != pn * pn:
                    raise ValueError(f'input_img_tokens: scale tensors must be (1 or B, pn^2) with pn in {self.patch_nums}, got {tuple(t.shape)}')
            if len({t.device for t in toks}) != 1:
                raise ValueError('input_img_tokens: every scale must be on one device')
            toks = torch.cat(toks, dim=1)
        elif not isinstance(toks, torch.Tensor) or toks.dim() != 2 or toks.shape[1] != self.L:
            raise ValueError(f'input_img_tokens must be the per-scale list of vae.img_to_idxBl or a (1 or B, {self.L}) tensor')
        if toks.shape[0] not in (1, B):
            raise ValueError(f'input_img_tokens must have 1 or B = {B} rows, got {toks.shape[0]}')
        if toks.dtype.is_floating_point or toks.dtype.is_complex or toks.dtype == torch.bool:
            raise ValueError('input_img_tokens must hold integer token ids')
        if toks.numel() and (int(toks.min()) < 0 or int(toks.max()) >= self.V):
            raise ValueError(f'input_img_tokens must lie in [0, {self.V})')
        return toks.long()

    def _edit_mask(self, mask, B: int) -> torch.Tensor:
        """edit_mask -> (1 or B, h, w) float32, as replace_embedding's .to(torch.float) converts it"""
        if not isinstance(mask, torch.Tensor) or mask.dtype.is_complex or mask.dim() not in (2, 3):
            raise ValueError('edit_mask must be a real or bool (h, w) or (B, h, w) tensor')
        if mask.dim() == 2:
            mask = mask.unsqueeze(0)
        if mask.shape[0] not in (1, B) or mask.shape[1] < 1 or mask.shape[2] < 1:
            raise ValueError(f'edit_mask must be (h, w) or (B = {B}, h, w) with h, w >= 1, got {tuple(mask.shape)}')
        return mask.to(torch.float32).contiguous()

    # ---- teacher-forced forward (PyTorch; reference var.py:118-124,192-234) ---------------------------------------------
    def get_logits(self, h_or_h_and_residual, cond_BD: Optional[torch.Tensor]):
        if not isinstance(h_or_h_and_residual, torch.Tensor):
            h, resi = h_or_h_and_residual
            h_or_h_and_residual = resi + self.blocks[-1].drop_path(h)
        return self.head(self.head_nm(h_or_h_and_residual.float(), cond_BD).float()).float()

    def forward(self, label_B: torch.LongTensor, x_BLCv_wo_first_l: torch.Tensor) -> torch.Tensor:
        """logits (B, L, V) for teacher-forced inputs (B, L-first_l, Cvae); block-causal mask instead of a KV cache"""
        if (not torch.is_grad_enabled() and not self.training and self.prog_si < 0 and self.lvl_1L.is_cuda and self.head.weight.dtype == torch.float32
                and self.C == 64 * self.num_heads and x_BLCv_wo_first_l is not None and x_BLCv_wo_first_l.shape[1] == self.L - self.first_l):
            # (train mode keeps the PyTorch branch below: DropPath / dropout are live there, reference helpers.py:39-59)
            # inference (no autograd): scale-by-scale over the KV cache on the HIP kernels, fp32, same label dropping as below
            label_B = torch.where(torch.rand(label_B.shape[0], device=label_B.device) < self.cond_drop_rate, self.num_classes, label_B)
            return self.engine().teacher_forced_logits(label_B, x_BLCv_wo_first_l)
        B = x_BLCv_wo_first_l.shape[0]
        with torch.autocast(device_type=x_BLCv_wo_first_l.device.type, enabled=False):
            label_B = torch.where(torch.rand(B, device=label_B.device) < self.cond_drop_rate, self.num_classes, label_B)
        return self._forward_torch(label_B, x_BLCv_wo_first_l)

    def _forward_torch(self, label_B: torch.LongTensor, x_BLCv_wo_first_l: torch.Tensor) -> torch.Tensor:
        """the PyTorch teacher-forced pass of forward() on labels as given (no condition dropping)"""
        bg, ed = self.begin_ends[self.prog_si] if self.prog_si >= 0 else (0, self.L)
        B = x_BLCv_wo_first_l.shape[0]
        with torch.autocast(device_type=x_BLCv_wo_first_l.device.type, enabled=False):
            cond_BD = self.class_emb(label_B)
            sos = cond_BD.unsqueeze(1).expand(B, self.first_l, -1) + self.pos_start.expand(B, self.first_l, -1)
            x = sos if self.prog_si == 0 else torch.cat((sos, self.word_embed(x_BLCv_wo_first_l.float())), dim=1)
            x = x + self.lvl_embed(self.lvl_1L[:, :ed].expand(B, -1)) + self.pos_1LC[:, :ed]
        mask = self.attn_bias_for_masking[:, :, :ed, :ed]
        cond_or_gss = self.shared_ada_lin(cond_BD)
        main_type = torch.matmul(x.new_ones(8, 8), x.new_ones(8, 8)).dtype       # follows an enclosing autocast, like the reference
        x, cond_or_gss, mask = x.to(main_type), cond_or_gss.to(main_type), mask.to(main_type)
        for blk in self.blocks:
            x = blk(x=x, cond_BD=cond_or_gss, attn_bias=mask)
        x = self.get_logits(x.float(), cond_BD)
        if self.prog_si == 0:      # keep word_embed in the graph for DDP
            x[0, 0, 0] += self.word_embed.weight[0, 0] * 0 + self.word_embed.bias[0] * 0
        return x

    @torch.no_grad()
    def token_log_likelihood(self, gt_tokens, label, cfg: float = 0.0, max_rows: int = 64) -> torch.Tensor:
        """(N, K, L) fp32: log p(gt token) of every image under every candidate class, teacher-forced.

        Fork API for VAR as a zero-shot classifier: one call replaces eval_prob.py:437-463 (bayesian mode: forward, log_softmax, gather, per
        candidate class) and, with cfg > 0, var_analysis.py:322-349 (z = (1+t)*cond - t*uncond, t = cfg * si/(S-1) per scale, one
        unconditional pass per image shared by all its classes).  gt_tokens: (N, L) int64, torch.cat(vae.img_to_idxBl(img), 1); label: (K,)
        (the same candidates for every image) or (N, K), a tensor or a list; labels in [0, num_classes] are used as given (no condition
        dropping, whatever cond_drop_rate is).  Classification: lp.sum(-1).argmax(-1); eval_prob --Clayer c: lp[..., cumsum[c]:].sum(-1).
        max_rows bounds the transformer rows of one pass (images_in_pass x (classes_in_pass + [cfg > 0])).
        On the HIP path (CUDA, eval mode, prog_si < 0, fp32 head, head_dim 64) the per-token values are reduced from each scale's logits by a
        gfx950 kernel: no (rows, L, V) tensor is made, the precision follows set_hip_precision / torch.autocast as forward() does.  Elsewhere
        the reference's formula runs in PyTorch."""
        gt, lab, cfg = self._scoring_args(gt_tokens, label, cfg, max_rows)
        if self._scoring_on_hip(gt):
            return self.engine().token_log_likelihood(gt, lab, cfg, int(max_rows))
        # the reference's formula (eval_prob.py:441-463; var_analysis.py:322-344), one image at a time
        out = []
        for i, logits in self._teacher_forced_torch(gt, lab, cfg, max_rows):
            lp = torch.nn.functional.log_softmax(logits, dim=-1)
            out.append(lp.gather(dim=-1, index=gt[i:i + 1, :logits.shape[1]].expand(lab.shape[1], -1).unsqueeze(-1)).squeeze(-1))
        return torch.stack(out, 0)

    @torch.no_grad()
    def token_scores(self, gt_tokens, label, score: str, cfg: float = 0.0, max_rows: int = 64, *, group: Optional[int] = None,
                     threshold: Optional[float] = None, top_k: Optional[int] = None) -> torch.Tensor:
        """(N, K, L) fp32 per-token class scores, teacher-forced: the fork's four scoring modes in one call each.

        gt_tokens, label, cfg and max_rows mean exactly what they mean in token_log_likelihood (same validation, packing and guided z).  With
        p = softmax(z) per token and the codes ordered by z descending, ties by ascending code index (a total order; torch.sort, which the
        fork uses, leaves the order of ties unspecified):
          'log_prob'           log p_gt: token_log_likelihood's values bit for bit (eval_prob.py bayesian).
          'group_smoothed'     group G (None -> the fork's 50, G >= 1): r = rank of gt, [lo, hi) = [r - r % G, min(lo + G, V)):
                               log(sum of p over the ranks [lo, hi) / (hi - lo) + 1e-10)   (eval_prob.py:37-92 smooth_bayesian).  Only which
                               group gt falls into depends on the tie order, not the values of a group.
          'neighbor_max'       threshold (finite, >= 0, required): max of log p_v over the codes v with d(gt, v) <= threshold; gt itself is
                               always in (eval_prob.py:389-393 fast_neighbor_bayesian, the rule of smooth_sampling's threshold mode at its last scale).
          'expected_distance'  -sum_v p_v d(gt, v); with top_k in [1, V] the sum runs over the top_k codes of the order above with their p
                               renormalised to sum to 1 (var_analysis.py:252-258 l2_dist, negated: higher is better).
        d is the direct-form L2 distance between codebook vectors, sqrt of one fma chain over the channels in channel order (the neighbour
        table's arithmetic), not torch.cdist's |a|^2 + |b|^2 - 2ab form.  A parameter given to a mode that does not use it, an
        unknown score or a parameter out of range raises ValueError.
        On the HIP path (the conditions of token_log_likelihood) each scale's logits are reduced by varhip_token_score_f32; the distance modes
        read the (V, V) table of SamplingEngine.code_distance_table (64 MiB at V = 4096, built once per codebook).  Elsewhere the same formulas
        run in PyTorch on the per-image logits."""
        desc = self._score_desc(score, group, threshold, top_k)
        if score == 'log_prob':
            return self.token_log_likelihood(gt_tokens, label, cfg, max_rows)
        gt, lab, cfg = self._scoring_args(gt_tokens, label, cfg, max_rows)
        if self._scoring_on_hip(gt):
            return self.engine().token_scores(gt, lab, cfg, int(max_rows), desc)
        cb = self.vae_proxy[0].quantize.embedding.weight.detach().float()
        out = []
        for i, z in self._teacher_forced_torch(gt, lab, cfg, max_rows):
            g = gt[i, :z.shape[1]]
            d = code_distance_rows(cb, g) if score != 'group_smoothed' else None
            out.append(token_score_torch(z.float(), g, desc, d))
        return torch.stack(out, 0)

    @torch.no_grad()
    def distance_profile(self, gt_tokens, label, edges, cfg: float = 0.0, max_rows: int = 64, *, min_prob: float = 0.0) -> DistanceProfile:
        """The distance-probability profile of the teacher-forced distributions -> DistanceProfile (histograms; see there).

        Replaces the fork's var_analysis.py:352-425 (plot_dist_kde: the (K, L, V) softmax, the gathered (K, L, V) codebook distances and the
        (d, p) pairs it subsamples to max_points) and the binning of those pairs at :694-732 / :798-818: for every ground-truth token, each
        code's probability p_v is paired with its codebook distance d(gt, v), and the pairs are reduced to a count and a probability mass per
        image, candidate class, scale and distance bin.  Every pair is counted: the curves are exact, not a random subsample.
        gt_tokens, label, cfg and max_rows mean exactly what they mean in token_scores (same validation, packing and guided z).  edges: B + 1
        fp32 values, 1 <= B <= 256, strictly increasing, edges[0] >= 0, the last may be +inf; bin b is edges[b] <= d < edges[b + 1].
        min_prob (finite, in [0, 1)): only pairs with p_v > min_prob count (the fork's `probs > 1e-10` style cut; 0 keeps every p_v > 0).
        d is the direct-form distance table of token_scores; p_v the fp32 softmax; the mass is summed in fixed point (2^-48), so the result is
        bit-equal across max_rows, packing, class order and repeated calls.  A bad edges or min_prob raises ValueError.
        On the HIP path (the conditions of token_log_likelihood) each scale's logits are reduced by varhip_dist_profile_f32 behind the head: no
        (rows, L, V) tensor is made.  Elsewhere distance_profile_torch runs on the per-image logits, at most max_rows class rows at a time."""
        gt, lab, cfg = self._scoring_args(gt_tokens, label, cfg, max_rows)
        e32, min_prob = self._profile_args(edges, min_prob)
        dev = gt.device
        N, K = lab.shape
        if self._scoring_on_hip(gt):
            mass, count = self.engine().distance_profile(gt, lab, cfg, int(max_rows), e32, min_prob)
            return DistanceProfile(count, mass, e32.to(dev), min_prob, self.patch_nums)
        nsc = len(self.patch_nums)
        B = e32.numel() - 1
        cb = self.vae_proxy[0].quantize.embedding.weight.detach().float()
        count = torch.zeros(N, K, nsc, B, dtype=torch.int64, device=dev)
        mass = torch.zeros(N, K, nsc, B, dtype=torch.int64, device=dev)
        for i, z in self._teacher_forced_torch(gt, lab, cfg, max_rows):
            d = code_distance_rows(cb, gt[i, :z.shape[1]])
            for si, (b, e) in enumerate(self.begin_ends):
                for k0 in range(0, K, int(max_rows)):
                    c, m = distance_profile_torch(z[k0:k0 + max_rows, b:e].float(), gt[i, b:e], d[b:e], e32, min_prob)
                    count[i, k0:k0 + max_rows, si], mass[i, k0:k0 + max_rows, si] = c, m
        return DistanceProfile(count, mass, e32.to(dev), min_prob, self.patch_nums)

    @torch.no_grad()
    def class_information(self, gt_tokens, label, cfg: float = 0.0, max_rows: int = 64, *, prior=None) -> ClassInformation:
        """Per token, how much the class changes the model's prediction -> ClassInformation (see there): the mutual information between the
        class and the next token under the teacher-forced prefix,
          I(c ; x_t | x_<t) = H(sum_k pi_k p_k) - sum_k pi_k H(p_k),
        the expected information a token carries about the class.  It needs no label of the image, lies in [0, H(pi)] and can be compared
        across scales, images and model depths; its (N, L) map feeds evidence_maps (ClassInformation.mi_map).
        gt_tokens, label, cfg and max_rows mean exactly what they mean in token_scores (same validation, packing and guided z); at most 16384
        candidates per image.  prior: None (uniform, 1 / K) or (K,) / (N, K) non-negative finite weights whose rows sum to 1 within 1e-6; they
        are rounded to fp32 and used as given (not renormalised).  A bad prior raises ValueError.
        On the HIP path (the conditions of token_log_likelihood) each scale's logits are reduced by varhip_class_mix_f32 behind the head: the
        (K, L, V) softmax tensor the definition asks for is never made.  When a pass holds all K classes of its images the mixture stays in
        LDS; otherwise (K + [cfg > 0] > max_rows) the chunks add into an (L, V) int64 accumulator per image and varhip_class_mix_finish_f32
        finalises each scale.  Elsewhere class_information_torch runs on the per-image logits, at most max_rows class rows at a time."""
        gt, lab, cfg = self._scoring_args(gt_tokens, label, cfg, max_rows)
        N, K = lab.shape
        if K > CLASS_INFO_MAX_CAND:
            raise ValueError(f'class_information takes at most {CLASS_INFO_MAX_CAND} candidates per image, got {K}')
        pri = self._prior_arg(prior, N, K).to(gt.device)
        if self._scoring_on_hip(gt):
            r = self.engine().class_information(gt, lab, cfg, int(max_rows), pri)
            return ClassInformation(r['entropy'], r['h_mix'], r['h_cond'], r['mi'], r['logp_mix'], pri, self.patch_nums)
        dev = gt.device
        ent = torch.empty(N, K, self.L, dtype=torch.float32, device=dev)
        per_tok = [torch.empty(N, self.L, dtype=torch.float32, device=dev) for _ in range(4)]
        for i, z in self._teacher_forced_torch(gt, lab, cfg, max_rows):
            for b, e in self.begin_ends:
                r = class_information_torch(z[:, b:e].float(), gt[i, b:e], pri[i], int(max_rows))
                ent[i, :, b:e] = r[0]
                for dst, src in zip(per_tok, r[1:]):
                    dst[i, b:e] = src
        return ClassInformation(ent, *per_tok, pri, self.patch_nums)

    @torch.no_grad()
    def attention_profile(self, gt_tokens, label, *, radius: int = 1, layers=None, max_rows: int = 64, return_tokens: bool = False) -> AttentionProfile:
        """What the attention layers do with their probability, by scale -> AttentionProfile (integer sums; see there).

        For every selected block, head and query: how much of softmax(q . k) goes to the keys of the query's own scale, how much to each earlier
        scale, and how much to the query's own neighbourhood (grid positions within Chebyshev distance `radius`).  These are the observations
        behind KV-cache pruning and scale skipping; taking them from softmax(QK^T) of reference basic_var.py:107-117 needs depth x H x L^2 floats
        per image.  gt_tokens: (N, L) integer tokens, teacher-forced as in token_log_likelihood; label: an int or (N,) class ids in [0,
        num_classes] (num_classes: unconditional), one condition per image; layers: None (all blocks) or strictly increasing block indices;
        radius: an int >= 0; max_rows bounds the images of one transformer pass; return_tokens also keeps every query's own shares.
        On the HIP path (the conditions of token_log_likelihood; f32 only: under a 16-bit precision ValueError) the blocks run on the KV cache
        and varhip_attn_profile_f32 reduces each selected block's queries against its key cache right behind it, with the scores of the
        sampler's attention kernel bit for bit: no (L, L) tensor is made, the head is skipped.  Elsewhere attention_profile_torch runs the module
        stack with the block-causal mask.  Both apply the same quantisation, so the integers agree up to what the two q / k differ by."""
        dev = self.lvl_1L.device
        gt = self._token_shape(gt_tokens)
        N = gt.shape[0]
        lab = A.labels_1d(label, N, f'label must be an int or (N,) integer class ids, N = {N}', scalar=True)
        A.integer(radius, 'radius must be an integer >= 0', 0)
        A.integer(max_rows, 'max_rows must be an integer >= 1', 1)
        layers = A.block_layers(layers, self.depth)
        self._token_label_range(gt, lab)
        gt, lab = gt.to(dev, torch.int64), lab.to(dev, torch.int64)
        radius = int(radius)
        r_eff = min(radius, max(self.patch_nums))                  # (beyond the largest grid every radius means the whole scale)
        if self._scoring_on_hip(gt):
            r = self.engine().attention_profile(gt, lab, r_eff, layers, int(max_rows), bool(return_tokens))
            return AttentionProfile(r['share_q'], r['nan_queries'], r['tokens'], self.patch_nums, radius, layers)
        if self.prog_si >= 0:
            raise ValueError('attention_profile covers every scale: prog_si must be < 0')
        share, nanq, tokens = attention_profile_torch(self, gt, lab, r_eff, layers, bool(return_tokens))
        return AttentionProfile(share, nanq, tokens, self.patch_nums, radius, layers)

    def _flow_args(self, gt_tokens, label, targets, layers, max_rows):
        """what attention_maps and attention_rollout check first -> (gt, lab on the device as int64, targets as flat indices, layers)"""
        dev = self.lvl_1L.device
        gt = self._token_shape(gt_tokens)
        N = gt.shape[0]
        lab = A.labels_1d(label, N, f'label must be an int or (N,) integer class ids, N = {N}', scalar=True)
        targets = A.flow_targets(targets, self.patch_nums)
        A.integer(max_rows, 'max_rows must be an integer >= 1', 1)
        layers = A.block_layers(layers, self.depth)
        self._token_label_range(gt, lab)
        return gt.to(dev, torch.int64), lab.to(dev, torch.int64), targets, layers

    @torch.no_grad()
    def attention_maps(self, gt_tokens, label, targets, *, layers=None, max_rows: int = 8) -> AttentionMaps:
        """Which positions of its own and of the coarser maps a token reads -> AttentionMaps (see there): for every target token, selected block
        and head the row softmax_j(q_t . k_j) of reference basic_var.py:107-117, without the depth x H x L^2 floats per image of the matrix.

        gt_tokens: (N, L) integer tokens, teacher-forced as in token_log_likelihood; label: an int or (N,) class ids in [0, num_classes];
        targets: 1 to 32 entries, each a flat token index in [0, L) or (scale, row, col), the same for every image; layers: None (all blocks)
        or strictly increasing block indices; max_rows bounds the images of one transformer pass (a pass keeps D' x L x C floats of queries per
        image).  On the HIP path (the conditions of token_log_likelihood; f32 only: under a 16-bit precision ValueError) the blocks run on the
        KV cache, every selected block's queries are kept for the call, and varhip_attn_rowstats_f32 / varhip_attn_flow_f32 form the rows with
        the scores of the sampler's attention kernel bit for bit.  Elsewhere attention_maps_torch forms the dense masked softmax per image in
        float64."""
        gt, lab, targets, layers = self._flow_args(gt_tokens, label, targets, layers, max_rows)
        if self._scoring_on_hip(gt):
            r = self.engine().attention_flow(gt, lab, targets, layers, int(max_rows))
            return AttentionMaps(r['rows'], r['nan_queries'], targets, layers, self.patch_nums)
        if self.prog_si >= 0:
            raise ValueError('attention_maps covers every scale: prog_si must be < 0')
        rows, nanq = attention_maps_torch(self, gt, lab, targets, layers)
        return AttentionMaps(rows, nanq, targets, layers, self.patch_nums)

    @torch.no_grad()
    def attention_rollout(self, gt_tokens, label, targets, *, layers=None, alpha: float = 0.5, max_rows: int = 8) -> AttentionRollout:
        """Where a token's information comes from through all selected blocks -> AttentionRollout (see there): attention rollout (Abnar &
        Zuidema 2020) of every target token, r <- (1 - alpha) r + alpha r Pbar_l from the last selected block to the first, r one-hot at the
        target, Pbar_l the head mean of block l's softmax(QK^T).  alpha in [0, 1] weighs the attention against the residual path (0.5: the
        paper's); the other arguments, the routes and the refusals are attention_maps'.  On the HIP path no (L, L) matrix is made: the row
        vectors are pushed through P tile by tile (varhip_attn_flow_f32), two launches per layer."""
        gt, lab, targets, layers = self._flow_args(gt_tokens, label, targets, layers, max_rows)
        alpha = A.rollout_alpha(alpha)
        if self._scoring_on_hip(gt):
            r = self.engine().attention_flow(gt, lab, targets, layers, int(max_rows), alpha)
            return AttentionRollout(r['flow'], r['nan_queries'], targets, layers, alpha, self.patch_nums)
        if self.prog_si >= 0:
            raise ValueError('attention_rollout covers every scale: prog_si must be < 0')
        flow, nanq = attention_rollout_torch(self, gt, lab, targets, layers, alpha)
        return AttentionRollout(flow, nanq, targets, layers, alpha, self.patch_nums)

    @torch.no_grad()
    def logit_lens(self, gt_tokens, label, *, layers=None, max_rows: int = 64) -> LogitLens:
        """At which depth the next-scale prediction forms -> LogitLens (per-token values; see there).

        The "logit lens": the trained head (head_nm + head, get_logits of reference var.py:118-124) applied to the residual stream behind every
        selected block, compared with the final prediction: per token and layer the loss, the entropy, KL(final || layer), the argmax and the
        rank of the ground-truth token.  Taking them from forward hooks needs depth x (N, L, V) logits and as many softmaxes.  gt_tokens: (N, L)
        integer tokens, teacher-forced as in evaluate; label: an int or (N,) class ids in [0, num_classes], used as given; layers: None (all
        blocks) or strictly increasing block indices; max_rows bounds the images of one transformer pass, and no value depends on it.
        On the HIP path (the conditions of token_log_likelihood; the precision follows set_hip_precision / torch.autocast, the residual stream
        and the logits are fp32 in all of them) each selected block's output is kept per scale, the head runs on it behind the final head, and
        varhip_token_lens_f32 reduces the two logits rows of a token to the five values: no per-layer logits tensor is made, and the last
        block's nll / pred / rank are evaluate's bit for bit.  Elsewhere logit_lens_torch runs the same definitions on hooked block outputs
        (with prog_si >= 0 over the scales 0 .. prog_si)."""
        dev = self.lvl_1L.device
        gt = self._token_shape(gt_tokens)
        N = gt.shape[0]
        lab = A.labels_1d(label, N, f'label must be an int or (N,) integer class ids, N = {N}', scalar=True)
        A.integer(max_rows, 'max_rows must be an integer >= 1', 1)
        layers = A.block_layers(layers, self.depth)
        self._token_label_range(gt, lab)
        gt, lab = gt.to(dev, torch.int64), lab.to(dev, torch.int64)
        if self._scoring_on_hip(gt):
            r = self.engine().logit_lens(gt, lab, layers, int(max_rows))
            return LogitLens(layers, r['nll'], r['entropy'], r['kl'], r['pred'], r['rank'], self.patch_nums)
        nsc = self.prog_si + 1 if self.prog_si >= 0 else len(self.patch_nums)
        return LogitLens(layers, *logit_lens_torch(self, gt, lab, layers, int(max_rows)), self.patch_nums[:nsc])

    @torch.no_grad()
    def logit_attribution(self, gt_tokens, label, *, target: str = 'gt', against=None, layers=None, max_rows: int = 64) -> LogitAttribution:
        """What every head and every MLP wrote into a token's final logit -> LogitAttribution (per-token terms; see there).

        Direct logit attribution: VAR's residual stream is a plain sum (reference basic_var.py:157-158) and its head an affine-free LayerNorm,
        a modulation and a linear map (var.py:118-124), so with the final token's deviation frozen the logit is linear in every summand of
        the stream and splits into one term per head, per proj bias, per MLP and for the embedding, in ONE teacher-forced pass per image.
        patch_effects answers another question (the total effect of removing a site, everything downstream included) with one row per site.
        gt_tokens: (N, L) integer tokens, teacher-forced as in evaluate; label: an int or (N,) class ids in [0, num_classes], used as given;
        target 'gt': the logit of the ground-truth token; 'margin': that logit minus the greatest other logit (the lowest index on ties);
        against: None or (N, L) integer rival tokens, which give the rival explicitly and imply the difference (a rival outside [0, V) is
        never dereferenced: that token's values are NaN and its rival -1); layers: None (all blocks) or strictly increasing block indices,
        the blocks whose terms are reported (`rest` collects the others); max_rows bounds the images of one transformer pass, and no value
        depends on it.
        On the HIP path (the conditions of token_log_likelihood; f32 only: under a 16-bit precision ValueError) every selected block's streams
        and proj input are kept per scale, and behind the scale's head varhip_dla_target_f32, varhip_dla_direction_f32, one C x C GEMM per
        selected block and varhip_rowdot_seg_f64 reduce them in float64: no tensor grows with the tokens, the blocks and the width at once.
        Elsewhere logit_attribution_torch runs the same definitions on hooked modules in the parameters' dtype (with prog_si >= 0 over the
        scales 0 .. prog_si)."""
        dev = self.lvl_1L.device
        gt = self._token_shape(gt_tokens)
        N = gt.shape[0]
        lab = A.labels_1d(label, N, f'label must be an int or (N,) integer class ids, N = {N}', scalar=True)
        max_rows = A.integer(max_rows, 'max_rows must be an integer >= 1', 1)
        layers = A.block_layers(layers, self.depth)
        target, against = A.attribution_target(target, against, N, self.L)
        self._token_label_range(gt, lab)
        gt, lab = gt.to(dev, torch.int64), lab.to(dev, torch.int64)
        against = None if against is None else against.to(dev, torch.int64)
        if self._scoring_on_hip(gt):
            r = self.engine().logit_attribution(gt, lab, target if against is None else 'against', against, layers, max_rows)
            return LogitAttribution(layers, self.patch_nums, **r)
        nsc = self.prog_si + 1 if self.prog_si >= 0 else len(self.patch_nums)
        r = logit_attribution_torch(self, gt, lab, target, against, layers, max_rows)
        rival = r.pop('rival')
        return LogitAttribution(layers, self.patch_nums[:nsc], rival, **{k: v.to(torch.float32) for k, v in r.items()})

    @torch.no_grad()
    def patch_effects(self, gt_tokens, label, sites=None, *, mode: str = 'mean', donor_label=None, scales=None, max_rows: int = 64) -> PatchEffects:
        """Which heads and MLPs an image's prediction depends on -> PatchEffects (per-token values; see there).

        Ablation and activation patching: per site one teacher-forced row in which the site's activation is replaced, compared with the clean
        row of the same image.  An elementary site is ('head', layer, head): that head's 64 columns of the attention output in front of proj
        (reference basic_var.py:117-119); ('attn', layer): all heads of the layer; ('mlp', layer): the MLP hidden activation behind the GELU,
        what fc2 reads.  An entry of `sites` is an elementary site or a tuple of them applied together in one row (a group of heads, a head
        and an MLP); None: every head, every 'attn' and every 'mlp' of the model, in that order.  mode 'zero' writes 0; 'mean' the mean over
        the tokens of the scale, per row and column; 'donor' the activation of the same tokens under donor_label (an int or (N,) class ids in
        [0, num_classes]; num_classes: the unconditional row), which shows through which sites the class reaches the tokens.  scales: None
        (the interventions apply at every scale) or the scale indices at which they apply while that scale is the query scale; later scales
        then see their effect through the keys and values.  gt_tokens: (N, L) integer tokens, teacher-forced as in evaluate; label: an int or
        (N,) class ids in [0, num_classes], used as given; max_rows bounds the rows of one transformer pass (an image's clean row, its donor
        row and at least one site row must fit), and no value depends on it.
        On the HIP path (the conditions of token_log_likelihood; f32 only: under a 16-bit precision ValueError) the rows of a sweep are ordinary
        rows of ordinary passes: varhip_act_patch_f32 rewrites the activation between two launches of the block, varhip_token_lens_f32 reduces
        every row against its image's clean row behind each scale's head, and no logits tensor is made; the clean row's nll / pred / rank are
        evaluate's bit for bit.  Elsewhere patch_effects_torch runs the same definitions on the module stack, one pass per row (with prog_si
        >= 0 over the scales 0 .. prog_si)."""
        dev = self.lvl_1L.device
        gt = self._token_shape(gt_tokens)
        N = gt.shape[0]
        lab = A.labels_1d(label, N, f'label must be an int or (N,) integer class ids, N = {N}', scalar=True)
        sites = A.patch_sites(sites, self.depth, self.num_heads)
        mode, donor, max_rows = A.patch_mode(mode, donor_label, N, max_rows)
        scales = A.patch_scales(scales, len(self.patch_nums))
        self._token_label_range(gt, lab)
        if donor is not None:
            A.in_range(donor, self.num_classes, f'donor_label must lie in [0, {self.num_classes}]')
            donor = donor.to(dev, torch.int64)
        gt, lab = gt.to(dev, torch.int64), lab.to(dev, torch.int64)
        columns = A.patch_columns(sites, self.C, self.blocks[0].ffn.fc1.weight.shape[0])
        if self._scoring_on_hip(gt):
            r = self.engine().patch_effects(gt, lab, columns, mode, donor, scales, max_rows)
            return PatchEffects(sites, mode, scales, r['nll'], r['entropy'], r['kl'], r['pred'], r['rank'], self.patch_nums, self.depth, self.num_heads)
        nsc = self.prog_si + 1 if self.prog_si >= 0 else len(self.patch_nums)
        nll, ent, kl, pred, rank = patch_effects_torch(self, gt, lab, columns, mode, donor, scales)
        return PatchEffects(sites, mode, scales, nll.float(), ent.float(), kl.float(), pred, rank, self.patch_nums[:nsc], self.depth, self.num_heads)

    @torch.no_grad()
    def attention_knockout(self, gt_tokens, label, edges=None, *, layers=None, heads=None, max_rows: int = 64) -> AttentionKnockout:
        """Which coarser scales a scale needs -> AttentionKnockout (per-token values; see there).

        attention_profile reports where the attention mass goes; mass is not dependence.  Here an edge of the block-causal graph is removed:
        per entry one teacher-forced row in which the queries of scale q may not read the keys (and values) of scale k, compared with the clean
        row of the same image.  An elementary edge is (q, k) with 0 <= k <= q < S, cut in the blocks of `layers` and the heads of `heads`
        (None: all; strictly increasing indices otherwise); (q, k, layer) and (q, k, layer, head) name one block, or one head of one block,
        instead.  The keys of scale k stay in the cache: later scales read them unless their own edge is cut too.  An entry of `edges` is an
        elementary edge or a tuple of them applied together in one row; None: every (q, k) with k < q, then (q, q) for q >= 1 (54 rows at 10
        scales).  ValueError before the tokens are touched for an entry that leaves some (query scale, block, head) without a visible key
        ((0, 0), or all of (q, 0) .. (q, q) together), that names an edge out of range, or that cuts the same edge twice.  gt_tokens: (N, L)
        integer tokens, teacher-forced as in evaluate; label: an int or (N,) class ids in [0, num_classes], used as given; max_rows (>= 2: the
        clean row and one entry's row) bounds the rows of one transformer pass, and no value depends on it.
        On the HIP path (the conditions of token_log_likelihood; f32 only: under a 16-bit precision ValueError) the rows of a sweep are
        ordinary rows of ordinary passes: where a row's mask is not full, varhip_attn_keysel_f32 runs the attention over the visible key scales
        only (hidden keys are not read), varhip_token_lens_f32 reduces every row against its image's clean row behind each scale's head, and
        no logits tensor is made; the clean row's nll / pred / rank are evaluate's bit for bit.  Elsewhere attention_knockout_torch runs the
        same definitions on the module stack, one pass per row (with prog_si >= 0 over the scales 0 .. prog_si)."""
        dev = self.lvl_1L.device
        gt = self._token_shape(gt_tokens)
        N = gt.shape[0]
        lab = A.labels_1d(label, N, f'label must be an int or (N,) integer class ids, N = {N}', scalar=True)
        layers, heads = A.block_layers(layers, self.depth), A.block_heads(heads, self.num_heads)
        edges = A.knockout_edges(edges, len(self.patch_nums), layers, heads, self.depth, self.num_heads)
        max_rows = A.integer(max_rows, 'max_rows must be an integer >= 2: the clean row and one row with a cut', 2)
        self._token_label_range(gt, lab)
        gt, lab = gt.to(dev, torch.int64), lab.to(dev, torch.int64)
        cuts = A.knockout_masks(edges, self.num_heads)
        if self._scoring_on_hip(gt):
            r = self.engine().attention_knockout(gt, lab, cuts, max_rows)
            return AttentionKnockout(edges, layers, heads, r['nll'], r['entropy'], r['kl'], r['pred'], r['rank'], self.patch_nums)
        nsc = self.prog_si + 1 if self.prog_si >= 0 else len(self.patch_nums)
        nll, ent, kl, pred, rank = attention_knockout_torch(self, gt, lab, cuts)
        return AttentionKnockout(edges, layers, heads, nll.float(), ent.float(), kl.float(), pred, rank, self.patch_nums[:nsc])

    @staticmethod
    def _prior_arg(prior, N: int, K: int) -> torch.Tensor:
        """the prior of class_information -> (N, K) fp32, contiguous, on the CPU or where it was given"""
        if prior is None:
            return torch.full((N, K), float(np.float32(1.0 / K)), dtype=torch.float32)
        try:
            p = torch.as_tensor(prior)
        except Exception:
            raise ValueError(f'prior must be None or ({K},) / ({N}, {K}) numbers') from None
        if p.dtype == torch.bool or p.is_complex() or p.dim() not in (1, 2) or p.shape[-1] != K or (p.dim() == 2 and p.shape[0] != N):
            raise ValueError(f'prior must be None or ({K},) / ({N}, {K}) numbers')
        p64 = p.detach().double()
        if p64.dim() == 1:
            p64 = p64.unsqueeze(0).expand(N, K)
        if not bool(torch.isfinite(p64).all()) or bool((p64 < 0).any()) or bool(((p64.sum(-1) - 1).abs() > 1e-6).any()):
            raise ValueError('prior must be finite and non-negative and every row must sum to 1 within 1e-6')
        return p64.float().contiguous()

    def evidence_maps(self, scores, *, scales=None, size: int = 256, image=None, image_range: str = 'pm1', alpha: float = 0.5,
                      return_maps: bool = False, check: bool = True) -> EvidenceMaps:
        """Where in the image the evidence for each class sits -> EvidenceMaps (see there): the spatial read-out of token_log_likelihood /
        token_scores, whose sum over tokens is all that classify uses.

        Replaces the fork's create_heatmaps_for_classes (eval_prob.py, inpainting.py, smoothing.py, var_analysis.py, var_size_analysis.py,
        drawn under --plot): a host loop over classes and scales with one F.interpolate each, K full-size maps and matplotlib on the CPU.
        scores: (N, K, L) or (K, L) fp32 per-token scores, L = sum(pn^2) of the model's patch_nums.  scales: an increasing tuple of scale
        indices, default the fork's first half range(S // 2).  The map of class k is
          m[n, k, y, x] = sum over the selected s of  w_s * bilinear_s(scores[n, k, scale s])(y, x),   w_s = float32(pn_s^2 / sum of selected pn^2)
        with torch's interpolate(mode='bilinear', align_corners=False) from pn_s x pn_s to size x size (no antialiasing below pn_s); the
        operation order is fixed, so the GPU and the PyTorch route agree bit for bit.
        image: (N, 3, size, size) or (3, size, size), in [-1, 1] (image_range='pm1') or [0, 1] ('01'): adds `overlays`, per class the jet
        colouring of (m - lo) / (hi - lo) blended as clip(img8 * (1 - alpha) + colour * alpha, 0, 255) the way the fork does in numpy.  (The
        fork computes the [-1, 1] -> [0, 1] step and then overwrites it, blending a wrapped image; that is not reproduced.)
        return_maps=True also returns the (N, K, size, size) maps.  check=True tests the selected scores for non-finite values on the
        device (one reduction and a host sync); with check=False a non-finite score leaves the result undefined.  Bad arguments raise ValueError.
        On a GPU tensor two gfx950 kernels do all of it: varhip_evidence_reduce_f32 loops over the classes per pixel tile and never writes
        the maps unless asked, varhip_evidence_overlay_u8 recomputes and colours them.  A CPU tensor takes evidence_maps_torch."""
        return evidence_maps(scores, self.patch_nums, scales=scales, size=size, image=image, image_range=image_range, alpha=alpha,
                             return_maps=return_maps, check=check)

    @torch.no_grad()
    def class_heatmaps(self, gt_tokens, label, image, score: str = 'log_prob', cfg: float = 0.0, max_rows: int = 64, **kw) -> EvidenceMaps:
        """token_scores(gt_tokens, label, score, cfg, max_rows) followed by evidence_maps(..., image=image): the fork's --plot in one call.
        Keyword arguments group / threshold / top_k go to token_scores, the rest (scales, size, image_range, alpha, return_maps, check) to
        evidence_maps.  No arithmetic of its own."""
        score_kw = {k: kw.pop(k) for k in ('group', 'threshold', 'top_k') if k in kw}
        return self.evidence_maps(self.token_scores(gt_tokens, label, score, cfg, max_rows, **score_kw), image=image, **kw)

    def _profile_args(self, edges, min_prob):
        """validation of distance_profile's edges and min_prob -> ((B + 1,) fp32 CPU tensor, the fp32 value of min_prob as a float)"""
        try:
            e = torch.as_tensor(edges).detach().to('cpu', torch.float32)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError('edges must be a 1-D ascending sequence or tensor of numbers') from None
        if e.dim() != 1 or not 2 <= e.numel() <= 257:
            raise ValueError('edges must be 1-D with B + 1 entries, 1 <= B <= 256')
        if bool(torch.isnan(e).any()) or float(e[0]) < 0 or not bool((e[1:] > e[:-1]).all()):
            raise ValueError('edges must be strictly increasing in fp32, without NaN, with edges[0] >= 0 (the last may be +inf)')
        A.real(min_prob, 'min_prob must be a finite number in [0, 1)', lambda v: 0.0 <= float(np.float32(v)) < 1.0)
        return e.contiguous(), float(np.float32(min_prob))

    def _score_desc(self, score, group, threshold, top_k) -> tuple:
        """validation of token_scores' score and its parameter -> the engine's score descriptor (mode, parameter)"""
        if score not in ('log_prob', 'group_smoothed', 'neighbor_max', 'expected_distance'):
            raise ValueError(f"score must be 'log_prob', 'group_smoothed', 'neighbor_max' or 'expected_distance', not {score!r}")
        uses = {'log_prob': (), 'group_smoothed': ('group',), 'neighbor_max': ('threshold',), 'expected_distance': ('top_k',)}[score]
        for name, val in (('group', group), ('threshold', threshold), ('top_k', top_k)):
            if val is not None and name not in uses:
                raise ValueError(f'{name} is not a parameter of score {score!r}')
        if score == 'group_smoothed':
            group = 50 if group is None else group
            A.integer(group, 'group must be an integer >= 1', 1, integral_float=True)
            desc = (score, int(group))
        elif score == 'neighbor_max':
            A.real(threshold, 'neighbor_max needs a finite threshold >= 0', lambda v: v >= 0, convert=threshold is not None)
            desc = (score, float(threshold))
        elif score == 'expected_distance':
            if top_k is not None:
                A.integer(top_k, f'top_k must be None or an integer in [1, {self.V}]', 1, self.V, integral_float=True)
            desc = (score, 0 if top_k is None else int(top_k))
        else:
            desc = (score,)
        return desc

    @torch.no_grad()
    def classify(self, gt_tokens, label, score: str = 'log_prob', cfg: float = 0.0, max_rows: int = 64, *, keep=None,
                 group: Optional[int] = None, threshold: Optional[float] = None, top_k: Optional[int] = None) -> ClassifyResult:
        """Zero-shot classification with per-scale class pruning -> ClassifyResult(pred, total, depth, tokens).

        gt_tokens, label, score, cfg, max_rows, group, threshold and top_k mean exactly what they mean in token_scores.  keep: None / {} (no
        pruning) or {scale: m}, 0 <= scale < S-1, integer m >= 1: after that scale each image keeps its m best surviving candidates (an m at or
        above the survivor count drops nothing).  The block-causal mask makes a candidate's scores through scale s final once computed, so
        pruned candidates are simply not scored further.
        Rule (a total order, used at every boundary and for pred): the float64 running total, highest first; NaN below everything (-inf
        included); ties by lower position in the image's label row (duplicate labels are distinct candidates).  The running total of a candidate
        scored through scale e is the float64 sum of its fp32 token scores 0 .. end(e)-1, added one by one in ascending token order
        (np.add.accumulate reproduces it bit for bit).
          tokens (N, K, L) fp32: the scored entries equal token_scores(...) bit for bit, in the same precision; every other entry is NaN
          depth  (N, K) int64: the last scale each candidate was scored through;  total (N, K) float64: its running total there
          pred   (N,) int64: the position of the best full-depth candidate under the rule (the class is label[n, pred[n]]); with keep=None the
                 rule's argmax of the full totals, lp.sum(-1).argmax(-1) with the ties and NaNs settled
        On the HIP path (the conditions of token_log_likelihood) the pruned candidates' later scales are never run: SamplingEngine.classify,
        at most 16384 candidates per image (more raise ValueError).  Elsewhere token_scores runs in full and the same rule is applied to its
        result: identical semantics, without the saving."""
        desc = self._score_desc(score, group, threshold, top_k)
        gt, lab, cfg = self._scoring_args(gt_tokens, label, cfg, max_rows)
        schedule = normalize_keep(keep, len(self.patch_nums), lab.shape[1])
        if self._scoring_on_hip(gt):
            return ClassifyResult(*self.engine().classify(gt, lab, cfg, int(max_rows), desc, schedule))
        kw = {k: v for k, v in (('group', group), ('threshold', threshold), ('top_k', top_k)) if v is not None}
        full = self.token_scores(gt, lab, score, cfg, max_rows, **kw)
        res = classify_rule(full.cpu().numpy(), [e for _, e in self.begin_ends], schedule)
        return ClassifyResult(*(torch.from_numpy(r).to(full.device) for r in res))

    def classify_generative(self, img, label, last_kept_scale: int, feature='vae_post', cfg: float = 0.0, max_rows: int = 64, *,
                            match_input_range: bool = False) -> GenerativeResult:
        """Generative zero-shot classification, the fork's `eval_prob.py --mode gen` (reference eval_prob.py:466-516), as one batched call
        -> GenerativeResult(pred, score, tokens).

        For each image and each candidate class: keep the image's tokens of scales 0 .. last_kept_scale, regenerate the later scales greedily
        under the class (var.inpainting(top_k=1, top_p=0, cfg=cfg)), decode, and score -mean|f_in - f_rec| between the features of the input
        image and of the reconstruction.  pred is the highest score; NaN ranks below everything, equal scores go to the lower position.
          img     (N, 3, 16P, 16P) fp32 in [-1, 1] (the fork's dataloader range); its tokens and feature are computed inside the call
          label   (K,) or (N, K) class ids in [0, num_classes] (num_classes: the unconditional class); duplicates are distinct candidates
          last_kept_scale  c, 0 <= c <= S-2: equals the fork's --Clayer c for c >= 1.  Divergence: the fork generates nothing for --Clayer 0
                  (Python falsiness; every class then ties), here c = 0 keeps scale 0 only
          feature 'vae_post' (quant_conv(encoder(x)), vae.img_to_post), 'vae_fhat' (vae.img_to_fhat(x)[-1]), or a callable f(images) -> (R, ...)
                  applied to the input images and to the reconstructions (the hook for dinov2 / CLIP / ResNet features users bring)
          cfg     the inpainting CFG schedule t = cfg * si / (S-1) (the fork's default is 4)
          max_rows  (image, class) rows per pass, packed across images; results are bitwise invariant to it
          match_input_range  False (default) reproduces the fork: the reconstruction handed to the feature is inpainting's output in [0, 1]
                  while the input image is in [-1, 1]; True hands it over in [-1, 1] (fhat_to_img's contract)
        Greedy rule: the lowest index among tied maxima of the CFG logits, no noise drawn (the fork's top_k=1 + torch.multinomial breaks exact
        fp32 ties with its Exp(1) draw), so the tokens equal var.inpainting(..., top_k=1, top_p=0) on every row without an exact tie; there
        is no g_seed.  Precision follows set_hip_precision as classify does ('auto': the caller's autocast); the transformer, decoder and
        encoder then run in it, and the scores are computed in fp32.  Scores are computed by varhip_feature_l1_f32 in a fixed order.
        Off the HIP path (a CPU model, training mode) RuntimeError, after the arguments are validated (ValueError)."""
        S = len(self.patch_nums)
        P = self.patch_nums[-1]
        x = img
        if (not isinstance(x, torch.Tensor) or x.dim() != 4 or x.dtype != torch.float32 or x.shape[0] < 1 or x.shape[1] != 3
                or x.shape[2] != 16 * P or x.shape[3] != 16 * P):
            raise ValueError(f'img must be an (N, 3, {16 * P}, {16 * P}) float32 tensor with N >= 1')
        N = x.shape[0]
        lab = A.labels_2d(label, N, f'label must be (K,) or (N, K) integer class ids with K >= 1, N = {N}')
        A.in_range(lab, self.num_classes, f'labels must lie in [0, {self.num_classes}]')
        c = A.integer(last_kept_scale, f'last_kept_scale must be an integer scale index in [0, {S - 2}], got {last_kept_scale!r}', 0, S - 2)
        if not callable(feature) and feature not in GENERATIVE_FEATURES:
            raise ValueError(f'feature must be one of {GENERATIVE_FEATURES} or a callable, got {feature!r}')
        cfg = A.cfg_arg(cfg)
        A.integer(max_rows, f'max_rows must be an integer >= {1 + (cfg > 0)}', 1 + (cfg > 0), integral_float=True)
        if not isinstance(match_input_range, bool):
            raise ValueError('match_input_range must be a bool')
        vae = self.vae_proxy[0]
        if not (self._scoring_on_hip(self.lvl_1L) and vae.quant_conv.kernel_size == (3, 3)):
            raise RuntimeError('VAR.classify_generative: this build runs the generative classifier on MI355X HIP kernels only (an eval-mode fp32 '
                               'model on a CUDA/ROCm device; no CPU fallback by design)')
        score, tokens = self.engine().classify_generative(x, lab.contiguous(), int(c), feature, cfg, int(max_rows), match_input_range)
        sc = score.cpu().numpy().astype(np.float64)
        pred = torch.tensor([int(rule_order(sc[n])[0]) for n in range(N)], dtype=torch.int64, device=score.device)
        return GenerativeResult(pred, score, tokens)

    @torch.no_grad()
    def evaluate(self, gt_tokens, label_B, *, label_smooth: float = 0.0, max_rows: int = 64) -> EvalResult:
        """The trainer's validation pass and logging metrics in one call -> EvalResult (sums; see there).

        Replaces reference trainer.py:54-84 (eval_ep: forward, cross entropy on all tokens and on the last scale, the two argmax accuracies)
        and :126-156 (the per-scale L_* / acc_* and z_voc_usage), and adds the rank of the ground-truth token (top-k accuracy for any k) and
        the label-smoothed objective.  gt_tokens: (N, L) integer tokens or the per-scale list of vae.img_to_idxBl(img); label_B: (N,) class
        ids in [0, num_classes], a tensor or a list.  max_rows bounds the images of one transformer pass; the per-token values and the integer
        sums do not depend on it.
        Deviation from the reference: its forward() drops labels at random with cond_drop_rate even in eval mode (var.py:199), so the numbers
        eval_ep prints are noisy; here the labels are used as given, as in token_log_likelihood.  A caller who wants the reference's numbers
        passes labels that are already dropped (num_classes).
        Per token, with z the fp32 logits row: nll = -log_softmax(z)[gt] (on the HIP path token_log_likelihood's value bit for bit, negated);
        pred = torch.argmax(z); rank = |{v : z_v > z_gt or (z_v == z_gt and v < gt)}|; the smoothing term z_gt - mean_v z_v with the mean
        taken in float64.
        On the HIP path (the conditions of token_log_likelihood) each scale's logits are reduced behind the head by varhip_token_eval_f32 and
        the sums by varhip_eval_reduce_f32 in a fixed order: no (N, L, V) logits tensor is made; the precision follows set_hip_precision /
        torch.autocast.  Elsewhere (CPU, train mode, prog_si >= 0) the same definitions run in PyTorch on _forward_torch's logits, at most
        max_rows images at a time; with prog_si >= 0 the result covers the scales 0 .. prog_si only."""
        gt, lab, label_smooth = self._eval_args(gt_tokens, label_B, label_smooth, max_rows)
        N, S = gt.shape[0], len(self.patch_nums)
        dev = gt.device
        if self._scoring_on_hip(gt):
            r = self.engine().evaluate(gt, lab, int(max_rows))
            tokens_S = torch.tensor([N * pn * pn for pn in self.patch_nums], dtype=torch.int64, device=dev)
            return EvalResult(N, r['nll_S'], r['smooth_S'], r['correct_S'], tokens_S, r['pred_hist_V'], r['nll_BL'], r['pred_BL'], r['rank_BL'],
                              label_smooth, self.patch_nums)
        nsc = self.prog_si + 1 if self.prog_si >= 0 else S
        ed = self.begin_ends[nsc - 1][1]
        x_all = self.vae_proxy[0].quantize.idxBl_to_var_input([gt[:, b:e] for b, e in self.begin_ends])[:, :ed - self.first_l]
        parts = []
        for i0 in range(0, N, int(max_rows)):
            z = self._forward_torch(lab[i0:i0 + max_rows], x_all[i0:i0 + max_rows]).float()
            parts.append(token_eval_torch(z, gt[i0:i0 + max_rows, :ed]))
        nll, smooth, pred, rank = (torch.cat(p) for p in zip(*parts))
        be = self.begin_ends[:nsc]
        return EvalResult(N, torch.stack([nll[:, b:e].double().sum() for b, e in be]), torch.stack([smooth[:, b:e].double().sum() for b, e in be]),
                          torch.stack([(rank[:, b:e] == 0).sum() for b, e in be]).to(torch.int64),
                          torch.tensor([N * (e - b) for b, e in be], dtype=torch.int64, device=dev),
                          torch.bincount(pred.reshape(-1), minlength=self.V), nll, pred, rank, label_smooth, self.patch_nums[:nsc])

    def _eval_args(self, gt_tokens, label_B, label_smooth, max_rows):
        """validation of evaluate -> (gt (N, L) int64, labels (N,) int64 on the model's device, label_smooth)"""
        dev = self.lvl_1L.device
        toks = gt_tokens
        if isinstance(toks, (list, tuple)) and len(toks) and all(isinstance(t, torch.Tensor) for t in toks):
            if len(toks) != len(self.patch_nums) or any(t.dim() != 2 or t.shape[0] != toks[0].shape[0] or t.shape[1] != pn * pn
                                                        for t, pn in zip(toks, self.patch_nums)):
                raise ValueError(f'gt_tokens: the per-scale list must hold {len(self.patch_nums)} tensors (N, pn^2) with pn in {self.patch_nums}')
            if len({t.device for t in toks}) != 1:
                raise ValueError('gt_tokens: every scale must be on one device')
            toks = torch.cat(list(toks), dim=1)
        gt = self._token_shape(toks)
        lab = A.labels_1d(label_B, gt.shape[0], f'label_B must be (N,) integer class ids, N = {gt.shape[0]}')
        A.real(label_smooth, 'label_smooth must be a finite number in [0, 1)', lambda v: 0.0 <= v < 1.0)
        A.integer(max_rows, 'max_rows must be an integer >= 1', 1)
        self._token_label_range(gt, lab)
        return gt.to(dev, torch.int64), lab.to(dev, torch.int64), float(label_smooth)

    def _scoring_args(self, gt_tokens, label, cfg, max_rows):
        """validation of token_log_likelihood / token_scores: -> (gt (N, L) int64, labels (N, K) int64 on the model's device, cfg)"""
        dev = self.lvl_1L.device
        gt = self._token_shape(gt_tokens)
        lab = A.labels_2d(label, gt.shape[0], f'label must be (K,) or (N, K) integer class ids with K >= 1, N = {gt.shape[0]}')
        cfg = A.cfg_arg(cfg)
        A.integer(max_rows, f'max_rows must be an integer >= {1 + (cfg > 0)} (the class rows of a pass plus the unconditional row with cfg > 0)', 1 + (cfg > 0),
                  integral_float=True)
        self._token_label_range(gt, lab)
        return gt.to(dev, torch.int64), lab.to(dev, torch.int64), cfg

    # ---- lossless token coding --------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def compress(self, gt_tokens, label_B, cfg: float = 0.0, scales: Optional[int] = None) -> CompressResult:
        """Code the tokens of B images losslessly with this model as the probability source: image b's blob is about -log2 p(tokens | label,
        coarser scales) bits long plus a 44 + 2 S byte header.  gt_tokens: (B, L) integer ids, or the list vae.img_to_idxBl returns; label_B:
        an int or (B,) class ids in [0, num_classes]; cfg: the guidance of the coding distribution (t = cfg * si / (S - 1) per scale, as in
        sampling; 0 = the conditional model); scales = s: only scales 0 .. s are coded (decompress can complete the rest greedily).
        The walk is sample()'s on 2B rows with the tokens given; per scale varhip_code_table_f32 turns every logits row into an integer
        frequency table (include/var_hip.h) and leaves the token's (C, F); the rANS coder runs on the host.  A blob does not depend on what it
        was batched with, nor on the calls made before.  f32 only (ValueError under a 16-bit precision); a CPU model: RuntimeError."""
        from .. import abi, hip
        dev = self._hip_only('compress')
        gt = self._token_shape(torch.cat(list(gt_tokens), 1) if isinstance(gt_tokens, (list, tuple)) else gt_tokens)
        B, S = gt.shape[0], len(self.patch_nums)
        lab = A.labels_1d(label_B, B, f'label_B must be an int or ({B},) integer class ids', scalar=True)
        cfg = A.cfg_arg(cfg)
        last = S - 1 if scales is None else A.integer(scales, f'scales must be None or an integer in [0, {S - 1}]', 0, S - 1, integral_float=True)
        self._token_label_range(gt, lab)
        pairs, flags = self.engine().code_tokens(gt.to(dev, torch.int64), lab.to(dev, torch.int64), cfg, last)
        n = self.begin_ends[last][1]
        if flags[:, :n].any():
            b, j = (int(v) for v in np.argwhere(flags[:, :n])[0])
            raise hip.VarHipError(f'compress: the coding table of image {b}, token {j} was refused (a NaN or no finite maximum in its logits row)')
        tok = gt.cpu().numpy()
        labs = lab.tolist()
        blobs, ideal = [], np.zeros((B, S), np.float64)
        buf, nw = np.empty(n + 2, np.uint32), np.zeros(1, np.int64)
        for b in range(B):
            hip.call_host('rans_encode_host', pairs[b], n, buf, n + 2, nw)
            blobs.append(codec_pack(buf[:int(nw[0])], labs[b], cfg, self.V, self.patch_nums, last + 1, codec_token_hash(tok[b, :n]), abi.CODEC_PB))
            bits = abi.CODEC_PB - np.log2(pairs[b, :n, 1].astype(np.float64))
            ideal[b, :last + 1] = [bits[b0:e0].sum() for b0, e0 in self.begin_ends[:last + 1]]
        return CompressResult(blobs, torch.tensor([len(x) for x in blobs], dtype=torch.int64), torch.from_numpy(ideal), tuple(self.patch_nums))

    @torch.no_grad()
    def decompress(self, blobs, complete: Optional[str] = None, fill_cfg: float = 1.5, decode: bool = True) -> DecompressResult:
        """The tokens (and images) back from VAR.compress's blobs, which may carry different labels and come from different compress calls; they
        must agree on cfg, the coded scales, PB and patch_nums and match this model's V and patch_nums (ValueError otherwise).  Blobs that code
        scales 0 .. s < S - 1: complete=None leaves the later tokens -1 (the image, if asked for, is the coarse f_hat's), complete='greedy'
        fills them with the argmax of the guided logits (guidance fill_cfg), the completion inpainting's greedy route gives for that prefix.
        The walk is sample()'s with the bitstream as the chooser (varhip_rans_decode_u32 behind varhip_code_table_f32), no host
        synchronisation inside it.  A blob that fails the decoder's bounds check, the end check or the token hash raises VarCodecError naming
        the image and the check: also what decoding with other weights gives.  f32 only; a CPU model: RuntimeError."""
        from .. import abi
        dev = self._hip_only('decompress')
        if complete not in (None, 'greedy'):
            raise ValueError("complete must be None or 'greedy'")
        blobs = list(blobs)
        if not blobs:
            raise ValueError('decompress: no blob given')
        heads = [codec_unpack(x) for x in blobs]
        h0 = heads[0]
        for i, h in enumerate(heads):
            if (h['cfg'], h['coded'], h['pb'], h['patch_nums']) != (h0['cfg'], h0['coded'], h0['pb'], h0['patch_nums']):
                raise ValueError(f'decompress: blob {i} differs from blob 0 in cfg, coded scales, PB or patch_nums: decode such blobs in separate calls')
        S = len(self.patch_nums)
        if h0['patch_nums'] != tuple(self.patch_nums) or h0['V'] != self.V or any(h['V'] != self.V for h in heads):
            raise ValueError(f"decompress: the blobs were coded for V = {h0['V']}, patch_nums = {h0['patch_nums']}; this model has {self.V}, {tuple(self.patch_nums)}")
        if h0['pb'] != abi.CODEC_PB or not 1 <= h0['coded'] <= S or not math.isfinite(h0['cfg']) or h0['cfg'] < 0:
            raise ValueError('decompress: the header names a table precision, scale count or cfg this build does not code with')
        fill_cfg = A.cfg_arg(fill_cfg, 'fill_cfg')
        lab = torch.tensor([h['label'] for h in heads], dtype=torch.int64)
        if int(lab.min()) < 0 or int(lab.max()) > self.num_classes:
            raise ValueError(f'labels must lie in [0, {self.num_classes}]')
        last = h0['coded'] - 1
        nw = np.array([h['words'].shape[0] for h in heads], np.int64)
        off = np.concatenate(([0], np.cumsum(nw)[:-1])).astype(np.int64)
        words = np.concatenate([h['words'] for h in heads]).astype(np.uint32)
        fill = fill_cfg if complete == 'greedy' and last < S - 1 else None
        tokens, img, state, err, refused = self.engine().decode_tokens(words, off, nw, lab.to(dev), h0['cfg'], last, fill, bool(decode))
        tok = tokens.cpu().numpy()
        n = self.begin_ends[last][1]
        for i, h in enumerate(heads):
            x, pos = int(state[i, 0]) | int(state[i, 1]) << 32, int(state[i, 2])
            if refused[i]:
                raise VarCodecError(i, 'table', f'{int(refused[i])} logits rows of the model hold a NaN or no finite maximum')
            if err[i]:
                raise VarCodecError(i, 'bounds', 'the decoder ' + {1: "read past the stream's last word", 2: 'met a slot that no symbol owns'}.get(int(err[i]), 'was given a word range outside the upload'))
            if x != 1 << 31 or pos != int(nw[i]):
                raise VarCodecError(i, 'end', f'after the last token the state is {x:#x} (expected 0x80000000) with {pos} of {int(nw[i])} words read')
            if codec_token_hash(tok[i, :n]) != h['hash']:
                raise VarCodecError(i, 'hash', 'the decoded tokens do not hash to the value in the header')
        return DecompressResult(tokens, img, lab.to(dev), last)

    def _token_shape(self, gt_tokens) -> torch.Tensor:
        """the token argument of the scoring calls and of evaluate -> an (N, L) integer tensor, shape and dtype checked"""
        return A.token_rows(gt_tokens, self.L)

    def _token_label_range(self, gt: torch.Tensor, lab: torch.Tensor):
        """explicit range checks (one host sync each): a bad token would index past a logits row, a bad label past class_emb"""
        A.token_label_range(gt, lab, self.V, self.num_classes)

    def _scoring_on_hip(self, gt: torch.Tensor) -> bool:
        return not self.training and self.prog_si < 0 and gt.device.type == 'cuda' and self.head.weight.dtype == torch.float32 and self.C == 64 * self.num_heads

    def _teacher_forced_torch(self, gt, lab, cfg, max_rows):
        """the reference's per-image teacher-forced logits (eval_prob.py:437-440; var_analysis.py:322-344 with cfg > 0): yields
        (image, (K, ed, V) z), z the guided combination when cfg > 0"""
        dev = gt.device
        N, K = lab.shape
        ed = self.begin_ends[self.prog_si][1] if self.prog_si >= 0 else self.L
        x_all = self.vae_proxy[0].quantize.idxBl_to_var_input([gt[:, b:e] for b, e in self.begin_ends])
        ratio = torch.tensor([si / self.num_stages_minus_1 if self.num_stages_minus_1 > 0 else 0.0 for si, pn in enumerate(self.patch_nums) for _ in range(pn * pn)],
                             device=dev)[:ed]
        t = cfg * ratio.unsqueeze(0).unsqueeze(-1)
        for i in range(N):
            x_i = x_all[i:i + 1]
            rows = []
            for k0 in range(0, K, max_rows):
                kk = lab[i, k0:k0 + max_rows]
                rows.append(self._forward_torch(kk, x_i.expand(kk.shape[0], -1, -1)).float())
            logits = torch.cat(rows, 0)
            if cfg > 0:
                uncond = self._forward_torch(torch.full((1,), self.num_classes, dtype=torch.int64, device=dev), x_i).float()
                logits = (1 + t) * logits - t * uncond
            yield i, logits

    @torch.no_grad()
    def inpainting(self, gt_tokens: torch.Tensor, mask: torch.Tensor, label: Optional[Union[int, torch.LongTensor]] = None,
                   g_seed: Optional[int] = None, cfg: float = 1.5, top_k: int = 0, top_p: float = 0.0, more_smooth: bool = False) -> torch.Tensor:
        """Fork API (reference var.py:236-364): resample the tokens where `mask` is False, keep `gt_tokens` where it is True;
        gt_tokens/mask are (B, L) as produced by vae.img_to_idxBl (concatenated).  Returns (B, 3, H, W) in [0, 1].
        Runs the same HIP loop as autoregressive_infer_cfg with the token replacement fused in (SamplingEngine.sample)."""
        if mask.shape != gt_tokens.shape:
            raise ValueError('Mask shape must match the latent token shape obtained from vae.img_to_idxBl')
        dev = self._hip_only('inpainting', how=' (no CPU fallback by design)')
        B = gt_tokens.shape[0]
        rng, lab = self._rng_and_labels(B, label, g_seed, negative_is_uncond=False, seeded_draw=False, name='label')
        # more_smooth (var.py:332-341): the embeddings then come from the gumbel softmax of the filtered logits alone — the kept tokens
        # only enter through the reference's `final_tokens`, which that branch never reads; defined only when no scale is fully kept
        return self.engine().sample(B, lab, rng, cfg, top_k, top_p, gt_tokens=gt_tokens, keep_mask=mask, more_smooth=bool(more_smooth))

    def smooth_sampling(self, gt_tokens: torch.Tensor, n: int, label: Optional[Union[int, torch.LongTensor]] = None,
                        g_seed: Optional[int] = None, cfg: float = 1.5, more_smooth: bool = False,
                        neighbor_threshold: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Fork API (reference var.py:367-572): every position takes, among the `n` nearest codebook neighbours of its
        ground-truth token (candidate-count mode: the first 1 + int((n-1)*ratio) of them; threshold mode: those within
        d_min + (neighbor_threshold - d_min)*ratio), the one with the highest CFG log-probability.
        Returns (image (B,3,H,W) in [0,1], sum of the chosen log-probabilities — each truncated to an integer first, as the
        reference's `sampled_tokens.new_tensor(max_vals)` does —, sum of log_softmax(-distance) at the chosen candidates).
        The neighbour table uses the direct-form L2 distance with ties broken by index (var_hip.h), where the reference's
        torch.cdist/argsort pair leaves both to the BLAS and an unstable sort."""
        dev = self._hip_only('smooth_sampling', how=' (no CPU fallback by design)')
        B = gt_tokens.shape[0]
        rng, lab = self._rng_and_labels(B, label, g_seed, negative_is_uncond=False, seeded_draw=False, name='label')
        eng = self.engine()
        img = eng.sample(B, lab, rng, cfg, 0, 0.0, more_smooth=more_smooth,
                         smooth=dict(gt=gt_tokens, n=n, thr=None if neighbor_threshold is None else float(neighbor_threshold)))
        sum_ll, sum_dist_ll = eng.last_smooth
        return img, sum_ll, sum_dist_ll

    # ---- initialisation (reference var.py:577-627) -------------------------------------------------------------------
    def init_weights(self, init_adaln=0.5, init_adaln_gamma=1e-5, init_head=0.02, init_std=0.02, conv_std_or_gain=0.02):
        if init_std < 0: init_std = (1 / self.C / 3) ** 0.5
        print(f'[init_weights] {type(self).__name__} with {init_std=:g}')
        for m in self.modules():
            if isinstance(m, (nn.Linear, nn.Embedding)):
                nn.init.trunc_normal_(m.weight.data, std=init_std)
                if getattr(m, 'bias', None) is not None: m.bias.data.zero_()
                if isinstance(m, nn.Embedding) and m.padding_idx is not None: m.weight.data[m.padding_idx].zero_()
            elif isinstance(m, (nn.LayerNorm, nn.GroupNorm)):
                if m.weight is not None: m.weight.data.fill_(1.)
                if m.bias is not None: m.bias.data.zero_()
        if init_head >= 0:
            self.head.weight.data.mul_(init_head); self.head.bias.data.zero_()
        self.head_nm.ada_lin[-1].weight.data.mul_(init_adaln); self.head_nm.ada_lin[-1].bias.data.zero_()
        for blk in self.blocks:
            blk.attn.proj.weight.data.div_(math.sqrt(2 * self.depth))
            blk.ffn.fc2.weight.data.div_(math.sqrt(2 * self.depth))
            if hasattr(blk, 'ada_lin'):
                lin = blk.ada_lin[-1]
                lin.weight.data[2 * self.C:].mul_(init_adaln); lin.weight.data[:2 * self.C].mul_(init_adaln_gamma); lin.bias.data.zero_()
            else:
                blk.ada_gss.data[:, :, 2:].mul_(init_adaln); blk.ada_gss.data[:, :, :2].mul_(init_adaln_gamma)
        self.invalidate_engine()           # `.data` edits bump no version counter: the HIP engine must re-read the weights

    def invalidate_engine(self):
        """Tell the HIP engine that parameters changed behind autograd's back (`p.data.copy_()`, EMA swaps, checkpoint surgery)."""
        if self._engine is not None:
            self._engine.invalidate()

    def load_state_dict(self, state_dict, strict=True, assign=False):
        ret = super().load_state_dict(state_dict, strict=strict, assign=assign)
        self.invalidate_engine()
        return ret

    def extra_repr(self):
        return f'drop_path_rate={self.drop_path_rate:g}'


try:
    from huggingface_hub import PyTorchModelHubMixin

    class VARHF(VAR, PyTorchModelHubMixin):
        def __init__(self, vae_kwargs, **kwargs):
            super().__init__(vae_local=VQVAE(**vae_kwargs), **kwargs)
except Exception:       # hub mixin is optional: it only adds from_pretrained / push_to_hub
    VARHF = None
