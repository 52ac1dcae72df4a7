"""What tests/test_distance_profile_cpu.py and tests/test_distance_profile_gpu.py share: VAR.distance_profile's definitions restated
independently in numpy, and the bar the fixed-point mass is held to.

Per row (one token of one class row) with fp32 logits z, token g and the fp32 distance row d = dist[g]:  p = softmax(z) evaluated in float64;
code v is in bin b iff edges[b] <= d_v < edges[b + 1] (np.searchsorted on the fp32 edges against the fp32 distances) and p_v > min_prob;
count[b] += 1 and mass[b] += p_v (np.add.at).  A NaN distance is in no bin; a row whose token lies outside [0, V) contributes nothing.

The bar on a cell's mass:  |mass - ref| <= 1e-5 * ref + count * 2^-48.  The first term is the bar DESIGN.md §12.1 asserts for sums of
non-negative terms that each carry a relative error of a few u = 2^-24 (the exponential, the subtraction of the maximum, the row sum, the
division); the second is twice the rounding of the fixed point, rint(p * 2^48) being off by at most 2^-49 per element."""
import numpy as np

Q = 2.0 ** 48
REL = 1e-5


def row_probs(z):
    """float64 softmax of fp32 rows z (R, V)"""
    z64 = np.asarray(z, dtype=np.float32).astype(np.float64)
    e = np.exp(z64 - z64.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def profile_rows(z, gt, dist, edges, min_prob=0.0):
    """z (R, V) fp32 logits, gt (R,) tokens, dist (>= V rows, >= V columns) fp32 table, edges (B + 1,) fp32 -> (count (R, B) int64, mass (R, B) float64)"""
    z = np.asarray(z, dtype=np.float32)
    R, V = z.shape
    gt = np.asarray(gt, dtype=np.int64).reshape(R)
    dist = np.asarray(dist, dtype=np.float32)
    edges = np.asarray(edges, dtype=np.float32)
    B = edges.shape[0] - 1
    thr = np.float64(np.float32(min_prob))
    p = row_probs(z)
    count, mass = np.zeros((R, B), np.int64), np.zeros((R, B), np.float64)
    for r in range(R):
        g = int(gt[r])
        if g < 0 or g >= V:
            continue
        d = dist[g, :V]
        b = np.searchsorted(edges, d, side='right') - 1                  # |{i : edges[i] <= d}| - 1 (a NaN sorts behind +inf: masked below)
        ok = (b >= 0) & (b < B) & ~np.isnan(d) & (p[r] > thr)
        np.add.at(count[r], b[ok], 1)
        np.add.at(mass[r], b[ok], p[r][ok])
    return count, mass


def profile(z, gt, dist, edges, min_prob=0.0):
    """one scale of a pass: z (images, classes, l, V) fp32, gt (images, l) -> (count, mass) (images, classes, B), summed over the l tokens"""
    z = np.asarray(z, dtype=np.float32)
    I, K, l, V = z.shape
    g = np.broadcast_to(np.asarray(gt, dtype=np.int64).reshape(I, 1, l), (I, K, l)).reshape(-1)
    c, m = profile_rows(z.reshape(-1, V), g, dist, edges, min_prob)
    return c.reshape(I, K, l, -1).sum(2), m.reshape(I, K, l, -1).sum(2)


def clear_of_threshold(z, gt, min_prob, rel=1e-4):
    """the condition on the INPUT under which count is comparable across precisions: no element of a scored row has a float64 probability
    within relative `rel` of min_prob (an fp32 p_v a few u off could otherwise fall on the other side of it)"""
    z = np.asarray(z, dtype=np.float32)
    V = z.shape[-1]
    z = z.reshape(-1, V)
    gt = np.asarray(gt, dtype=np.int64).reshape(-1)
    p = row_probs(z[(gt >= 0) & (gt < V)])
    thr = np.float64(np.float32(min_prob))
    return not bool((np.abs(p - thr) <= rel * thr).any())


def mass_ok(got_mass_q, got_count, ref_count, ref_mass):
    """counts equal and |mass_q * 2^-48 - ref| <= 1e-5 * ref + count * 2^-48 in every cell -> (ok, message)"""
    got_mass_q, got_count = np.asarray(got_mass_q, dtype=np.int64), np.asarray(got_count, dtype=np.int64)
    if not np.array_equal(got_count, ref_count):
        bad = np.argwhere(got_count != ref_count)
        return False, f'count differs in {len(bad)} cells, first {tuple(bad[0])}: {got_count[tuple(bad[0])]} vs {ref_count[tuple(bad[0])]}'
    excess = np.abs(got_mass_q.astype(np.float64) / Q - ref_mass) - (REL * ref_mass + ref_count / Q)
    worst = np.unravel_index(int(np.argmax(excess)), excess.shape) if excess.size else ()
    rel = float(np.max(np.abs(got_mass_q.astype(np.float64) / Q - ref_mass) / np.maximum(ref_mass, 1e-300))) if excess.size else 0.0
    return bool((excess <= 0).all()), f'max relative mass error {rel:.3e}; worst cell {worst} exceeds the bar by {float(excess.max()) if excess.size else 0.0:.3e}'
