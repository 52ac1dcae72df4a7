"""The argument checkers of VAR's public calls (var.py): plain functions without model state.  Each returns the normalised value or raises
ValueError with the message the caller gives.

The definitions, once:
  integer   a Python int or a numpy integer, never a bool.  Where a call has always taken a float of integral value (`integral_float`)
            whatever equals its own int() passes too.
  float     int, float or a numpy scalar, never a bool, finite; `convert` marks the arguments that have always gone through float()
            (cfg, fill_cfg, threshold: a str or a 0-d tensor passes).  cfg and fill_cfg, and the per-image cfg / top_p, take a bool
            too (float(True) = 1.0): they always did, in every call.
  labels    an integer tensor (no float, complex or bool dtype) of the stated shape, in [0, num_classes] (num_classes: unconditional)
  tokens    an (N, L) integer tensor in [0, V)
  per image a scalar for all, or B values as a tensor, an ndarray, a list or a tuple
The range checks cost one host synchronisation per tensor (one aminmax)."""
import math

import numpy as np
import torch


def is_int(x) -> bool:
    return isinstance(x, (int, np.integer)) and not isinstance(x, bool)


def integer(x, msg: str, lo=None, hi=None, integral_float: bool = False) -> int:
    ok = is_int(x)
    if not ok and integral_float and not isinstance(x, bool):
        try:
            ok = bool(int(x) == x)
        except (TypeError, ValueError, OverflowError):
            ok = False
    if not ok or (lo is not None and x < lo) or (hi is not None and x > hi):
        raise ValueError(msg)
    return int(x)


def real(x, msg: str, ok=None, convert: bool = False) -> float:
    """a finite float that satisfies ok(value)"""
    try:
        if isinstance(x, bool) or not (convert or isinstance(x, (int, float, np.integer, np.floating))):
            raise TypeError
        v = float(x)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(msg) from None
    if not math.isfinite(v) or (ok is not None and not ok(v)):
        raise ValueError(msg)
    return v


def as_list(x):
    """a tensor or ndarray as the (nested) list of its values; anything else as it is"""
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().tolist()
    return x.tolist() if isinstance(x, np.ndarray) else x


def per_image(x, name: str, B: int, conv=None, each: int = 1) -> list:
    """a scalar for all or B values -> a list of B * each values (each: consecutive copies of an image's value), converted by conv"""
    x = as_list(x)
    if isinstance(x, (list, tuple)):
        if len(x) != B:
            raise ValueError(f'{name} must be a scalar or {B} values, got {len(x)}')
        vals = [v for v in x for _ in range(each)]
    else:
        vals = [x] * (B * each)
    try:
        return vals if conv is None else [conv(v) for v in vals]
    except (TypeError, OverflowError) as e:
        raise ValueError(f'{name}: {e}') from None


def _integral(v) -> int:
    if isinstance(v, bool) or (isinstance(v, float) and v != int(v)) or not isinstance(v, (int, float, np.integer)):
        raise ValueError(f'expected an integer, got {v!r}')
    return int(v)


def _integer_tensor(t: torch.Tensor) -> bool:
    return not (t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool)


def labels_1d(label, N, msg: str, scalar: bool = False) -> torch.Tensor:
    """(N,) integer class ids (N None: one or more); scalar: an int stands for N of them"""
    lab = torch.full((N,), int(label), dtype=torch.int64) if scalar and is_int(label) else torch.as_tensor(label)
    if lab.dim() != 1 or lab.numel() != (N if N is not None else max(lab.numel(), 1)) or not _integer_tensor(lab):
        raise ValueError(msg)
    return lab


def labels_2d(label, N: int, msg: str) -> torch.Tensor:
    """(K,) for every image or (N, K) integer class ids, K >= 1 -> (N, K)"""
    lab = torch.as_tensor(label)
    if lab.dim() == 1:
        lab = lab.unsqueeze(0).expand(N, -1)
    if lab.dim() != 2 or lab.shape[0] != N or lab.shape[1] < 1 or not _integer_tensor(lab):
        raise ValueError(msg)
    return lab


def in_range(t: torch.Tensor, hi: int, msg: str):
    """every element in [0, hi]: one host synchronisation"""
    lo, top = torch.stack(torch.aminmax(t)).tolist()
    if lo < 0 or top > hi:
        raise ValueError(msg)


def token_rows(gt_tokens, L: int) -> torch.Tensor:
    """the token argument of the scoring calls, of evaluate and of compress -> an (N, L) integer tensor, shape and dtype checked"""
    gt = torch.as_tensor(gt_tokens)
    if gt.dim() != 2 or gt.shape[1] != L or gt.shape[0] < 1 or not _integer_tensor(gt):
        raise ValueError(f'gt_tokens must be an (N, {L}) integer tensor of token ids')
    return gt


def token_label_range(gt: torch.Tensor, lab: torch.Tensor, V: int, num_classes: int):
    """explicit range checks (one host sync each): a bad token would index past a logits row, a bad label past class_emb"""
    in_range(gt, V - 1, f'gt_tokens must lie in [0, {V})')
    in_range(lab, num_classes, f'labels must lie in [0, {num_classes}]')


def block_layers(layers, depth: int) -> tuple:
    """the `layers` of attention_profile and logit_lens -> the selected block indices, ascending: None means every block"""
    if layers is None:
        return tuple(range(depth))
    try:
        layers = tuple(layers)
    except TypeError:
        raise ValueError('layers must be None or a strictly increasing sequence of block indices') from None
    if not layers or not all(is_int(b) for b in layers) \
            or any(b < 0 or b >= depth for b in layers) or any(b1 <= b0 for b0, b1 in zip(layers, layers[1:])):
        raise ValueError(f'layers must be None or a strictly increasing sequence of block indices in [0, {depth})')
    return tuple(int(b) for b in layers)


FLOW_MAX_TARGETS = 32


def flow_targets(targets, patch_nums) -> tuple:
    """the `targets` of attention_maps and attention_rollout -> 1 .. 32 flat token indices: an entry is a flat index in [0, L) or a
    (scale, row, col) triple of a scale's grid"""
    pns = tuple(patch_nums)
    L = sum(pn * pn for pn in pns)
    msg = (f'targets must be 1 to {FLOW_MAX_TARGETS} entries, each a flat token index in [0, {L}) or (scale, row, col) with scale in '
           f'[0, {len(pns)}) and row, col inside that scale\'s grid')
    targets = as_list(targets)
    if is_int(targets):
        targets = [targets]
    if not isinstance(targets, (list, tuple)) or not 1 <= len(targets) <= FLOW_MAX_TARGETS:
        raise ValueError(msg)
    out = []
    for t in targets:
        t = as_list(t)
        if is_int(t):
            if not 0 <= t < L:
                raise ValueError(msg)
            out.append(int(t))
        elif isinstance(t, (list, tuple)) and len(t) == 3 and all(is_int(v) for v in t):
            si, y, x = (int(v) for v in t)
            if not 0 <= si < len(pns) or not 0 <= y < pns[si] or not 0 <= x < pns[si]:
                raise ValueError(msg)
            out.append(sum(pn * pn for pn in pns[:si]) + y * pns[si] + x)
        else:
            raise ValueError(msg)
    return tuple(out)


def rollout_alpha(alpha) -> float:
    """attention_rollout's alpha: the weight of the attention against the residual path, in [0, 1]"""
    return real(alpha, 'alpha must be a number in [0, 1]', lambda v: 0.0 <= v <= 1.0)


ATTRIBUTION_TARGETS = ('gt', 'margin')


def attribution_target(target, against, N: int, L: int) -> tuple:
    """the `target` and `against` of VAR.logit_attribution -> (target, against as an (N, L) integer tensor or None).  The rival's range is
    not checked: an out-of-range rival is answered per token (NaN, rival -1), never dereferenced"""
    if target not in ATTRIBUTION_TARGETS:
        raise ValueError(f"target must be one of {ATTRIBUTION_TARGETS}, got {target!r}")
    if against is None:
        return target, None
    riv = torch.as_tensor(against)
    if riv.dim() != 2 or tuple(riv.shape) != (N, L) or not _integer_tensor(riv):
        raise ValueError(f'against must be None or an ({N}, {L}) integer tensor of rival token ids')
    return target, riv


PATCH_MODES = ('zero', 'mean', 'donor')


def _patch_site(site, depth: int, H: int) -> tuple:
    """one elementary site of VAR.patch_effects, checked: ('head', layer, head) | ('attn', layer) | ('mlp', layer)"""
    forms = "('head', layer, head), ('attn', layer) or ('mlp', layer)"
    if not isinstance(site, (tuple, list)) or not site or site[0] not in ('head', 'attn', 'mlp') or len(site) != (3 if site[0] == 'head' else 2):
        raise ValueError(f'sites: {site!r} is not {forms}')
    if not is_int(site[1]) or not 0 <= site[1] < depth:
        raise ValueError(f'sites: {tuple(site)!r}: the layer must be an integer in [0, {depth})')
    if site[0] == 'head' and (not is_int(site[2]) or not 0 <= site[2] < H):
        raise ValueError(f'sites: {tuple(site)!r}: the head must be an integer in [0, {H})')
    return (site[0],) + tuple(int(v) for v in site[1:])


def patch_sites(sites, depth: int, H: int) -> tuple:
    """the `sites` of VAR.patch_effects -> a tuple of entries, each a tuple of elementary sites applied together in one row.  None: every
    head, every 'attn' and every 'mlp' of the model, in that order; an entry is an elementary site or a non-empty sequence of them, which
    may not name a column twice (a site twice, or a head beside the 'attn' of its layer)"""
    if sites is None:
        return tuple((('head', b, h),) for b in range(depth) for h in range(H)) + tuple((('attn', b),) for b in range(depth)) \
            + tuple((('mlp', b),) for b in range(depth))
    if isinstance(sites, (str, bytes, dict)) or not hasattr(sites, '__iter__'):
        raise ValueError('sites must be None or a sequence of sites')
    out = []
    for entry in sites:
        if isinstance(entry, (tuple, list)) and entry and isinstance(entry[0], str):
            entry = (entry,)
        if not isinstance(entry, (tuple, list)) or not entry:
            raise ValueError(f'sites: {entry!r} is neither a site nor a non-empty tuple of sites')
        group = tuple(_patch_site(e, depth, H) for e in entry)
        for i, e in enumerate(group):
            for f in group[:i]:
                if e == f or (e[1] == f[1] and {e[0], f[0]} == {'head', 'attn'}):
                    raise ValueError(f'sites: {e!r} and {f!r} of one entry name the same columns')
        out.append(group)
    if not out:
        raise ValueError('sites must be None or hold at least one site')
    return tuple(out)


def patch_columns(sites: tuple, C: int, hidden: int) -> tuple:
    """normalised sites -> per entry the column ranges (matrix 'att' | 'hid', layer, c0, c1) of varhip_act_patch_f32's directives: a head's 64
    columns of the attention output in front of proj, all C of them, or the whole MLP hidden activation"""
    col = lambda e: ('att', e[1], 64 * e[2], 64 * e[2] + 64) if e[0] == 'head' else ('att', e[1], 0, C) if e[0] == 'attn' else ('hid', e[1], 0, hidden)
    return tuple(tuple(col(e) for e in group) for group in sites)


def patch_scales(scales, S: int) -> tuple:
    """the `scales` of VAR.patch_effects -> the scale indices at which the interventions apply, ascending: None means every scale"""
    if scales is None:
        return tuple(range(S))
    try:
        scales = tuple(scales)
    except TypeError:
        raise ValueError('scales must be None or a sequence of scale indices') from None
    if not scales or not all(is_int(s) and 0 <= s < S for s in scales) or len(set(scales)) != len(scales):
        raise ValueError(f'scales must be None or distinct scale indices in [0, {S}), got {scales!r}')
    return tuple(sorted(int(s) for s in scales))


def patch_mode(mode, donor_label, N: int, max_rows) -> tuple:
    """mode, donor_label and max_rows of VAR.patch_effects -> (mode, donor labels (N,) integer tensor or None, max_rows)"""
    if mode not in PATCH_MODES:
        raise ValueError(f'mode must be one of {PATCH_MODES}, got {mode!r}')
    if (mode == 'donor') != (donor_label is not None):
        raise ValueError("donor_label goes with mode='donor', and only with it")
    donor = None if donor_label is None else labels_1d(donor_label, N, f'donor_label must be an int or (N,) integer class ids, N = {N}', scalar=True)
    least = 2 + (mode == 'donor')
    what = 'the donor row, the clean row and one site row' if mode == 'donor' else 'the clean row and one site row'
    return mode, donor, integer(max_rows, f'max_rows must be an integer >= {least}: {what}', least)


def block_heads(heads, H: int) -> tuple:
    """the `heads` of VAR.attention_knockout -> the selected head indices, ascending: None means every head"""
    if heads is None:
        return tuple(range(H))
    try:
        heads = tuple(heads)
    except TypeError:
        raise ValueError('heads must be None or a strictly increasing sequence of head indices') from None
    if not heads or not all(is_int(h) and 0 <= h < H for h in heads) or any(h1 <= h0 for h0, h1 in zip(heads, heads[1:])):
        raise ValueError(f'heads must be None or a strictly increasing sequence of head indices in [0, {H})')
    return tuple(int(h) for h in heads)


def _knockout_edge(edge, S: int, layers: tuple, heads: tuple, depth: int, H: int) -> tuple:
    """one elementary edge of VAR.attention_knockout, checked -> (q, k, blocks, heads): (q, k) in the call's layers and heads, (q, k, layer) in
    one block, (q, k, layer, head) in one head of one block (a None in either place: the call's)"""
    forms = '(q, k), (q, k, layer) or (q, k, layer, head)'
    if not isinstance(edge, (tuple, list)) or not 2 <= len(edge) <= 4:
        raise ValueError(f'edges: {edge!r} is not {forms}')
    q, k = edge[0], edge[1]
    if not is_int(q) or not is_int(k) or not 0 <= k <= q < S:
        raise ValueError(f'edges: {tuple(edge)!r}: the scales must be integers with 0 <= k <= q < {S}')
    bi = edge[2] if len(edge) > 2 else None
    h = edge[3] if len(edge) > 3 else None
    if bi is not None and (not is_int(bi) or not 0 <= bi < depth):
        raise ValueError(f'edges: {tuple(edge)!r}: the layer must be None or an integer in [0, {depth})')
    if h is not None and (not is_int(h) or not 0 <= h < H):
        raise ValueError(f'edges: {tuple(edge)!r}: the head must be None or an integer in [0, {H})')
    return int(q), int(k), layers if bi is None else (int(bi),), heads if h is None else (int(h),)


def knockout_edges(edges, S: int, layers: tuple, heads: tuple, depth: int, H: int) -> tuple:
    """the `edges` of VAR.attention_knockout -> a tuple of entries, each a tuple of elementary edges (q, k, blocks, heads) applied together in one
    row.  None: every (q, k) with k < q, then (q, q) for q >= 1, in the call's layers and heads.  An entry is an elementary edge or a non-empty
    sequence of them; it may not cut the same (q, k, block, head) twice, and it must leave every (query scale, block, head) a visible key (scale 0
    sees only itself; cutting (q, 0) .. (q, q) together hides everything)"""
    if edges is None:
        edges = [(q, k) for q in range(S) for k in range(q)] + [(q, q) for q in range(1, S)]
    if isinstance(edges, (str, bytes, dict)) or not hasattr(edges, '__iter__'):
        raise ValueError('edges must be None or a sequence of edges')
    out = []
    for entry in edges:
        if isinstance(entry, (tuple, list)) and entry and not isinstance(entry[0], (tuple, list)):
            entry = (entry,)
        if not isinstance(entry, (tuple, list)) or not entry:
            raise ValueError(f'edges: {entry!r} is neither an edge nor a non-empty tuple of edges')
        group = tuple(_knockout_edge(e, S, layers, heads, depth, H) for e in entry)
        cut = {}
        for q, k, bs, hs in group:
            for bi in bs:
                for h in hs:
                    seen = cut.setdefault((q, bi, h), set())
                    if k in seen:
                        raise ValueError(f'edges: {entry!r} cuts ({q}, {k}) twice in block {bi}, head {h}: duplicate edges')
                    seen.add(k)
        for (q, bi, h), ks in cut.items():
            if len(ks) == q + 1:
                raise ValueError(f'edges: {entry!r} leaves the queries of scale {q} without a visible key in block {bi}, head {h}')
        out.append(group)
    if not out:
        raise ValueError('edges must be None or hold at least one edge')
    return tuple(out)


def knockout_masks(entries: tuple, H: int) -> tuple:
    """normalised edges -> per entry {(query scale, block): [H key-scale masks]}: bit i of a mask set = key scale i is visible; only the
    (scale, block) pairs an entry touches appear, each with the full mask (bits 0 .. q) for the heads it leaves alone"""
    out = []
    for group in entries:
        m = {}
        for q, k, bs, hs in group:
            for bi in bs:
                row = m.setdefault((q, bi), [(2 << q) - 1] * H)
                for h in hs:
                    row[h] &= ~(1 << k)
        out.append({key: tuple(v) for key, v in m.items()})
    return tuple(out)


def cfg_arg(cfg, name: str = 'cfg') -> float:
    """cfg / fill_cfg: whatever float() takes, a bool included (1.0 / 0.0), as in the per-image samplers"""
    return real(float(cfg) if isinstance(cfg, bool) else cfg, f'{name} must be finite and >= 0', lambda v: v >= 0, convert=True)


def sample_args(V: int, label_B, g_seeds, cfg, top_k, top_p):
    """the argument handling of the per-image calls -> (labels (B,) integer tensor, seeds, cfgs, top_ks, top_ps: lists of B values)"""
    lab = labels_1d(label_B, None, 'label_B must hold B >= 1 integer class ids')
    B = lab.numel()
    if isinstance(g_seeds, (int, np.integer)) or (isinstance(g_seeds, torch.Tensor) and g_seeds.dim() == 0):
        raise ValueError(f'g_seeds must hold one seed per image ({B} values)')
    seeds = per_image(g_seeds, 'g_seeds', B, _integral)
    cfgs, ks, ps = per_image(cfg, 'cfg', B, float), per_image(top_k, 'top_k', B, _integral), per_image(top_p, 'top_p', B, float)
    if any(sd < 0 or sd >= 1 << 63 for sd in seeds):
        raise ValueError('g_seeds must lie in [0, 2^63)')
    if not all(math.isfinite(c) for c in cfgs):
        raise ValueError('cfg must be finite')
    if any(k < 0 or k > V for k in ks):
        raise ValueError(f'top_k must lie in [0, {V}]')
    if not all(0.0 <= p <= 1.0 for p in ps):                 # (NaN fails the comparison)
        raise ValueError('top_p must lie in [0, 1]')
    return lab, seeds, cfgs, ks, ps


def scheduled(x, name: str, S: int, B: int, integral: bool = False) -> np.ndarray:
    """a knob of VAR.sample_controlled -> (S, B) float64 (integral: int64): a scalar, (B,) per image, or (S, B) per scale and image; a B axis
    of size 1 broadcasts, so (S, 1) is a pure per-scale schedule"""
    shapes = f'a scalar, ({B},), ({S}, {B}) or ({S}, 1)'
    try:
        a = np.array(as_list(x))
        if a.dtype == bool or a.dtype == object or not (np.issubdtype(a.dtype, np.integer) or np.issubdtype(a.dtype, np.floating)):
            raise TypeError
        a = a.astype(np.float64)
    except (TypeError, ValueError):
        raise ValueError(f'{name} must be {shapes} of numbers') from None
    if not (a.ndim == 0 or (a.ndim == 1 and a.shape[0] in (1, B)) or (a.ndim == 2 and a.shape[0] == S and a.shape[1] in (1, B))):
        raise ValueError(f'{name} must be {shapes}, got shape {tuple(a.shape)}')
    a = np.broadcast_to(a, (S, B))
    if integral:
        if not np.isfinite(a).all() or (a != np.floor(a)).any():
            raise ValueError(f'{name} must hold integers')
        return a.astype(np.int64)
    return a.copy()


def control_args(V: int, S: int, B: int, cfg, top_k, top_p, temperature, min_p, logit_bias) -> dict:
    """the knobs of VAR.sample_controlled, each a scalar, (B,) or (S, B) with a size-1 B axis broadcasting (`scheduled`); logit_bias None, (V,),
    (B, V) or (S, B, V), again with a size-1 B -> dict(cfg, top_p (S, B) float64; top_k (S, B) int64; tau, min_p (S, B) float32, checked as the
    float32 values the sampler reads; bias: None or a float32 array that broadcasts to (S, B, V))"""
    out = dict(cfg=scheduled(cfg, 'cfg', S, B), top_k=scheduled(top_k, 'top_k', S, B, integral=True), top_p=scheduled(top_p, 'top_p', S, B))
    if not np.isfinite(out['cfg']).all():
        raise ValueError('cfg must be finite')
    if (out['top_k'] < 0).any() or (out['top_k'] > V).any():
        raise ValueError(f'top_k must lie in [0, {V}]')
    if not ((out['top_p'] >= 0.0) & (out['top_p'] <= 1.0)).all():                 # (NaN fails the comparison)
        raise ValueError('top_p must lie in [0, 1]')
    with np.errstate(over='ignore'):
        tau = scheduled(temperature, 'temperature', S, B).astype(np.float32)
        mp = scheduled(min_p, 'min_p', S, B).astype(np.float32)
    if (tau == 0).any():
        raise ValueError('temperature must be finite and > 0 (as a float32); for the limit temperature -> 0, greedy selection, use top_k=1')
    if not (np.isfinite(tau) & (tau > 0)).all():
        raise ValueError('temperature must be finite and > 0')
    if not ((mp >= 0) & (mp <= 1)).all():
        raise ValueError('min_p must lie in [0, 1]')
    out.update(tau=tau, min_p=mp, bias=None)
    if logit_bias is not None:
        shapes = f'({V},), ({B}, {V}), ({S}, {B}, {V}) or ({S}, 1, {V})'
        try:
            lb = np.array(as_list(logit_bias), dtype=np.float32)
        except (TypeError, ValueError):
            raise ValueError(f'logit_bias must be {shapes} of numbers') from None
        if not (lb.ndim in (1, 2, 3) and lb.shape[-1] == V and (lb.ndim < 2 or lb.shape[-2] in (1, B)) and (lb.ndim < 3 or lb.shape[0] == S)):
            raise ValueError(f'logit_bias must be {shapes}, got shape {tuple(lb.shape)}')
        if np.isnan(lb).any() or (lb == np.inf).any():
            raise ValueError('logit_bias must hold no NaN and no +inf (-inf bans a code)')
        if not (lb > -np.inf).any(axis=-1).all():
            raise ValueError('logit_bias bans every code of a row: each row needs at least one entry above -inf')
        out['bias'] = lb
    return out


COMPOSE_MAX_CLASSES = 8              # classes per image of VAR.sample_composed (varhip_mix_sample_rows_f32 takes up to 9 row groups)


def compose_args(V: int, num_classes: int, S: int, labels, weights, g_seeds, cfg, top_k, top_p, max_rows):
    """the argument handling of VAR.sample_composed -> (labels (B, K) int64 tensor, weights (S, B, K) float64 ndarray, and sample_args' seeds,
    cfgs, top_ks, top_ps: lists of B values).  labels: (B, K) integer class ids in [0, num_classes], 1 <= K <= 8; weights: (B, K) (every
    scale the same) or (S, B, K), finite, any sign; max_rows: an integer that holds one image's K + 1 rows"""
    lab = torch.as_tensor(labels)
    if lab.dim() != 2 or lab.shape[0] < 1 or not 1 <= lab.shape[1] <= COMPOSE_MAX_CLASSES or not _integer_tensor(lab):
        raise ValueError(f'labels must be a (B, K) integer tensor of class ids, B >= 1, 1 <= K <= {COMPOSE_MAX_CLASSES}')
    B, K = lab.shape
    in_range(lab, num_classes, f'labels must lie in [0, {num_classes}]')
    try:
        w = np.array(as_list(weights), dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f'weights must be a ({B}, {K}) or ({S}, {B}, {K}) array of numbers') from None
    if w.shape == (B, K):
        w = np.broadcast_to(w, (S, B, K)).copy()
    if w.shape != (S, B, K):
        raise ValueError(f'weights must be ({B}, {K}) or ({S}, {B}, {K}), got {tuple(w.shape)}')
    if not np.isfinite(w).all():
        raise ValueError('weights must be finite')
    integer(max_rows, f'max_rows must be an integer >= K + 1 = {K + 1}: the rows of one image', K + 1, integral_float=True)
    return (lab.long(), w) + sample_args(V, lab[:, 0], g_seeds, cfg, top_k, top_p)[1:]


def candidate_args(V: int, fields, label_B, g_seeds, n, by, cfg, top_k, top_p, max_images, noun=None):
    """the front end of sample_best_of, sample_best_of_pruned and sample_smc: n candidates (particles) per image, g_seeds (B, n), labels and
    parameters one per image -> (B, n, and sample_args' result on the B * n rows, the seeds as B rows).  noun: refuse n > max_images"""
    if by not in fields:
        raise ValueError(f'by must be one of {fields}, got {by!r}')
    integer(max_images, 'max_images must be an integer >= 1', 1, integral_float=True)
    sd = as_list(g_seeds)
    lab0 = torch.as_tensor(label_B)
    if (not isinstance(sd, (list, tuple)) or len(sd) != lab0.numel() or len(sd) < 1 or not all(isinstance(r, (list, tuple)) and len(r) == len(sd[0]) for r in sd)
            or len(sd[0]) < 1):
        raise ValueError('g_seeds must be (B, n): one row of n >= 1 seeds per image')
    B, width = len(sd), len(sd[0])
    try:
        agree = n is None or (not isinstance(n, bool) and int(n) == width)
    except (TypeError, ValueError, OverflowError):
        agree = False
    if not agree:
        raise ValueError(f'n = {n} but g_seeds holds {width} seeds per image')
    n = width
    if lab0.dim() != 1:
        raise ValueError('label_B must hold B >= 1 integer class ids')
    if noun is not None and n > max_images:
        raise ValueError(f'max_images = {max_images} holds no whole image of n = {n} {noun}')
    spread = lambda x: per_image(x, 'cfg / top_k / top_p', B, None, n)          # one value per image -> one per candidate
    return (B, n) + sample_args(V, lab0.repeat_interleave(n), [v for r in sd for v in r], spread(cfg), spread(top_k), spread(top_p)) + (sd,)


def _scale_index(si, S: int, what: str) -> int:
    return integer(si, f'{what}: a boundary must be an integer scale index in [0, {S - 2}], got {si!r}', 0, S - 2)


def normalize_resample(resample, S: int) -> list:
    """the `resample` argument of VAR.sample_smc -> the boundary scales as a list: integer scale indices in [0, S-2] (below the last scale),
    ascending and unique, validated as normalize_keep validates a scale; an empty sequence is allowed"""
    if resample is None or isinstance(resample, (str, bytes, dict)) or not hasattr(resample, '__iter__'):
        raise ValueError('resample must be a sequence of boundary scale indices')
    out = []
    for si in resample:
        _scale_index(si, S, 'resample')
        if out and si <= out[-1]:
            raise ValueError(f'resample: the boundaries must be ascending and unique, got {si!r} after {out[-1]}')
        out.append(int(si))
    return out


def normalize_keep(keep, S: int, alive: int) -> list:
    """the `keep` argument of VAR.classify and VAR.sample_best_of_pruned -> [(scale, m), ...] ascending in the scale.  keep: None / {} (no pruning)
    or {scale: m}, 0 <= scale < S-1, integer m >= 1; `alive` candidates enter.  A boundary that drops nothing (m at or above the survivor count
    before it) is no boundary and vanishes."""
    if keep is None:
        keep = {}
    if not isinstance(keep, dict):
        raise ValueError('keep must be None or a dict {scale_index: m}')
    sched = [(_scale_index(si, S, 'keep'), integer(m, f'keep: the number of candidates kept must be an integer >= 1, got {m!r}', 1)) for si, m in keep.items()]
    schedule = []
    for si, m in sorted(sched):
        if m < alive:                        # a boundary that drops nothing is no boundary
            schedule.append((si, m))
            alive = m
    return schedule


def counterfactual_args(V: int, L: int, S: int, num_classes: int, gt_tokens, label_src, label_dst, g_seeds, cfg, cfg_dst, top_k, top_p, first_scale,
                        max_images):
    """the argument handling of VAR.abduct_noise (label_dst None) and VAR.counterfactual -> dict(gt (B, L) integer tensor, lab_src (B,),
    lab_dst (B, K) or None, seeds, cfg: lists of B values; cfg_dst, top_k, top_p: lists of B * K values, request (b, k) at b * K + k; first,
    max_images).  label_dst: (B,) — K = 1 — or (B, K); cfg_dst None: the source's cfg; cfg_dst, top_k and top_p per image, shared by its K
    replays.  first_scale: an integer in [0, S] (S: nothing is abducted, nothing can change)."""
    gt = token_rows(gt_tokens, L)
    B = gt.shape[0]
    lab_src, seeds, cfgs = sample_args(V, label_src, g_seeds, cfg, 0, 0.0)[:3]
    if lab_src.numel() != B:
        raise ValueError(f'label_src must hold one class id per image ({B}), got {lab_src.numel()}')
    token_label_range(gt, lab_src, V, num_classes)
    first = integer(first_scale, f'first_scale must be an integer in [0, {S}], got {first_scale!r}', 0, S)
    most = integer(max_images, 'max_images must be an integer >= 1', 1, integral_float=True)
    out = dict(gt=gt, lab_src=lab_src, lab_dst=None, seeds=seeds, cfg=cfgs, first=first, max_images=most)
    if label_dst is None:
        return out
    lab = torch.as_tensor(label_dst)
    if lab.dim() == 1:
        lab = lab.unsqueeze(1)
    if lab.dim() != 2 or lab.shape[0] != B or lab.shape[1] < 1 or not _integer_tensor(lab):
        raise ValueError(f'label_dst must be ({B},) or ({B}, K) integer class ids, K >= 1')
    in_range(lab, num_classes, f'labels must lie in [0, {num_classes}]')
    K = lab.shape[1]
    spread = lambda x, name: per_image(x, name, B, None, K)
    _, _, cd, ks, ps = sample_args(V, lab.reshape(-1), [0] * (B * K), spread(cfgs if cfg_dst is None else cfg_dst, 'cfg_dst'), spread(top_k, 'top_k'),
                                   spread(top_p, 'top_p'))
    out.update(lab_dst=lab, cfg_dst=cd, top_k=ks, top_p=ps)
    return out
