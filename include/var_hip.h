/* var_hip.h — C ABI of libvar_hip.so: the MI355X (gfx950) kernels of VAR's next-scale sampling path.
 *
 * The reference (culiver/VAR) is pure Python on PyTorch: it has no FFI layer.  The drop-in boundary is the
 * `models` nn.Module API; *under* it the build calls this library through ctypes (var_amd/hip.py).  Each entry
 * point below names the reference code it replaces (paths relative to the reference repo).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (torch tensors); the library never allocates or
 *     frees caller-visible memory and keeps no state besides the optional timing table;
 *   - all matrices are row-major fp32; "ld*" are leading dimensions in elements;
 *   - `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream); launches are asynchronous;
 *   - return value: 0 on success, VARHIP_EINVAL (-1) for a shape/argument the kernels do not support,
 *     -(1000+hipError_t) when the launch itself failed.  No exceptions cross the ABI.
 *   - the CPU oracle (oracle/var_oracle.c) exports the same functions with prefix `varref_` and no stream
 *     argument, on HOST pointers: tests drive both with the same arguments.
 *   - arithmetic contract: dot products are k-ascending fp32 fma chains starting
 *     from 0 (what v_mfma_f32_32x32x2_f32 computes), then bias, then epilogue, each separately rounded.
 */
#ifndef VAR_HIP_H
#define VAR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VARHIP_EINVAL (-1)

typedef void* varhip_stream_t;

/* library / build info: returns a static string "var_hip <version> gfx950" */
const char* varhip_version(void);

/* ---- GEMM ------------------------------------------------------------------------------------------------
 * out[b][m][n] = epi( sum_k A[b][m][k] * W[b][n][k] + bias )          (torch F.linear: x @ W^T + b)
 * replaces: F.linear at basic_var.py:93 (mat_qkv), :119 (proj), :52 (fc1/fc2), :147,:170 (ada_lin), var.py:124
 * (head), and the 1x1 convs of basic_vae.py:53,69,71,83,89 (nin_shortcut, qkv, proj_out, the two bmm's).
 *   epi = VARHIP_EPI_NONE : acc + bias
 *         VARHIP_EPI_GELU : gelu_tanh(acc + bias)                              (basic_var.py:40,52)
 *         VARHIP_EPI_RESID: resid[m][n] + (acc + bias) * gamma[m / rows_per_group][n]   (basic_var.py:157-158);
 *                           gamma == NULL means no scaling: resid + (acc + bias)       (basic_vae.py:60,92)
 *   bias may be NULL.  bias_per_row != 0: bias is indexed by m instead of n.
 *   batch >= 1 with element strides sA/sW/sO (sW or sA may be 0 to share an operand); resid/gamma only with batch==1.
 * Fast path: K % 32 == 0, lda/ldw/sA/sW % 4 == 0, 16-byte aligned A/W and each operand of one batch element spanning < 4 GiB
 * (rows are addressed as 32-bit byte offsets from a scalar base); anything else takes an element-wise-load variant. */
#define VARHIP_EPI_NONE 0
#define VARHIP_EPI_GELU 1
#define VARHIP_EPI_RESID 2
int varhip_gemm_nt_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias,
                       float* out, int64_t ldo, int M, int N, int K, int epi,
                       const float* resid, int64_t ldr, const float* gamma, int64_t ldg, int rows_per_group,
                       int bias_per_row, int batch, int64_t sA, int64_t sW, int64_t sO, varhip_stream_t stream);
/* testing / experiments (host globals, no launch): force the tile of the following varhip_gemm_nt_f32 calls (0: 128x128, 1: 128x64, 2: 64x64,
 * 3: 32x32 with the 8-stage pipeline; -1: automatic choice; starts from the environment variable VARHIP_GEMM_TILE).  Applies only where the
 * fast path's conditions hold: a call that needs the element-wise-load variant still takes it.  Every tile computes the same bits. */
int varhip_gemm_force_tile(int tile);
/* the same for varhip_gemm_qkv_f32 below (0: 128-row tile, 1: 64-row tile; -1: automatic; starts from VARHIP_QKV_TILE) */
int varhip_gemm_qkv_force_tile(int tile);
/* the path the latest varhip_gemm_nt_f32 (0..2: the tiles above, 4: the 32x32 tile, 3: the element-wise-load variant) or varhip_gemm_qkv_f32
 * (0 / 1) call dispatched to; -1 before any call and unchanged by a call that returned VARHIP_EINVAL or had M == 0 */
int varhip_gemm_last_pick(void);
/* whether the latest varhip_gemm_nt_f32 call on one of the four tiles could use 16-byte accesses in its epilogue: 1, or 0 where N % 4, ldo % 4,
 * sO % 4, ldr % 4 (with resid), ldg % 4 (with gamma) or a misaligned out, column bias, resid or gamma forbids them (the results are the same
 * bits either way, so only this reports the choice); -1 before any call, after the element-wise-load variant and after varhip_gemm_qkv_f32 */
int varhip_gemm_last_evec(void);

/* y[i] = x[i] * sigmoid(x[i])   — the SiLU in front of every ada_lin (basic_var.py:147,170; var.py:80) */
int varhip_silu_f32(const float* x, float* y, int64_t n, varhip_stream_t stream);

/* out[b][j] = base[j] + cond[b][j], j < n   — shared AdaLN: ada_gss + cond_BD (basic_var.py:153-154) */
int varhip_add_bcast_f32(const float* base, const float* cond, float* out, int rows, int n, varhip_stream_t stream);

/* ---- AdaLN -----------------------------------------------------------------------------------------------
 * out[m][:] = LN(x[m][:]) * (scale[g][:] + 1) + shift[g][:],  g = m / rows_per_group, LN without affine,
 * biased variance, eps inside the sqrt.   replaces basic_var.py:157,158,174 (ln_wo_grad(...).mul(scale.add(1)).add_(shift)) */
int varhip_ln_modulate_f32(const float* x, const float* scale, int64_t ld_scale, const float* shift, int64_t ld_shift,
                           float* out, int M, int C, int rows_per_group, float eps, varhip_stream_t stream);

/* ---- q/k/v post-processing + KV-cache append ------------------------------------------------------------
 * qkv: [B2*l][3*C] (q | k | v, each H heads x 64).  For every row and head:
 *   l2norm != 0: q = q/max(|q|,1e-12) * exp(min(scale_mul[h], ln 100)),  k = k/max(|k|,1e-12)   (basic_var.py:101-105)
 *   l2norm == 0: q = q * plain_scale (attention scale folded into q; basic_var.py:72,117), k unchanged
 * q -> q_out[B2*l][C]; k,v -> caches [B2][H][Lmax][64] at positions pos0 .. pos0+l-1 (replaces the torch.cat
 * cache growth of basic_var.py:107-109 by an in-place append). */
int varhip_qkv_prep_f32(const float* qkv, const float* scale_mul, float plain_scale, int l2norm,
                        float* q_out, float* kcache, float* vcache,
                        int B2, int l, int H, int pos0, int Lmax, varhip_stream_t stream);

/* ---- mat_qkv GEMM with that post-processing fused into its epilogue -------------------------------------
 * Equivalent, bit for bit, to varhip_gemm_nt_f32(A, W[3C][K], bias[3C]) -> qkv[M][3C] followed by varhip_qkv_prep_f32,
 * without the [M][3C] round trip through HBM.   replaces basic_var.py:93 (F.linear with the q_bias|zero_k_bias|v_bias
 * concatenation) through :109.  Requires M == B2*l, C == H*64, K % 32 == 0, lda/ldw % 4 == 0, 16-byte aligned pointers and
 * A and W each spanning < 4 GiB (VARHIP_EINVAL otherwise). */
int varhip_gemm_qkv_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias, int M, int C, int K,
                        const float* scale_mul, float plain_scale, int l2norm,
                        float* q_out, float* kcache, float* vcache,
                        int B2, int l, int H, int pos0, int Lmax, varhip_stream_t stream);

/* ---- attention of l new queries over curL cached keys (no mask: block-causal by construction) -----------
 * out[b][t][h*64+c] = sum_j softmax_j(q[b][t][h] . k[b][h][j]) v[b][h][j][c],  j < curL
 * replaces slow_attn / flash_attn_func / memory_efficient_attention at basic_var.py:111-117 (head_dim 64, scale 1:
 * the scale is already folded into q by varhip_qkv_prep_f32).
 * Arithmetic contract (what makes the GPU result reproducible bit for bit by oracle/var_oracle.c):
 *   - the running-maximum recurrence over tiles of 32 keys: m' = max(m, max_tile s), a = e(m - m'), l = l a + sum p, O = O a + P V,
 *     p = e(s - m'), with e = vm_exp_le0 of include/var_math.h;
 *   - every dot product (64 channels of q.k; the 32 keys of a tile in p.v) is one fp32 fma chain in the 4-interleaved order
 *     0,4,1,5,2,6,3,7, 8,12,9,13, ... (inside each group of eight: j, j+4) — the order in which an MFMA 32x32x2 consumes operands
 *     that both lane halves read as 16 contiguous bytes;
 *   - l is kept as four partial sums over the keys with equal ((key >> 2) & 1, key & 1), ascending, added as (S00 + S01) + (S10 + S11);
 *   - out = O * (1 / l). */
int varhip_attn_cached_f32(const float* q, const float* kcache, const float* vcache, float* out,
                           int B2, int l, int H, int curL, int Lmax, varhip_stream_t stream);
/* testing / experiments (host global, no launch): the waves per workgroup (NW of k_attn_cached<NW>; a wave owns 32 queries, the grid is
 * ceil(l / (32 NW)) x H x B2) of the following varhip_attn_cached_f32 launches, varhip_adaln_block_f32's included: 1 .. 4 forces that NW,
 * 0 (and anything else) leaves the choice to the dispatch, which never launches a wave without queries; starts from the environment
 * variable VARHIP_ATTN_WAVES.  A query's arithmetic depends on its own wave's 32 queries and on the tile walk only: every NW computes the same bits. */
int varhip_attn_force_waves(int nw);
/* testing: the NW of the latest varhip_attn_cached_f32 launch, written by the launcher from the value it switches on.  0 before the first
 * launch; a refused call (VARHIP_EINVAL) leaves it unchanged.  Host only: it launches nothing and reads no device memory. */
int varhip_attn_last_waves(void);
/* ---- attention over a per-(row, head) subset of the key scales (VAR.attention_knockout) ----------------------------------
 * The operands of varhip_attn_cached_f32, with the cache cut into S1 key scales by ends (a HOST array with the rules of
 * varhip_attn_profile_f32: strictly increasing, ends[0] >= 1, ends[S1-1] == curL, S1 in [1, 16]; scale i holds the keys ends[i-1] <= j < ends[i])
 * and keymask, a DEVICE array of B2 * H words: bit i of keymask[b * H + h] set = row b, head h sees key scale i; bits at or above S1 are ignored.
 * Contract: the visible keys of (b, h), in ascending cache order, form a logical sequence of n = sum over visible i of (ends[i] - ends[i-1])
 * keys, and out[b][:][h] is what varhip_attn_cached_f32 computes on a cache that holds exactly those keys and values at positions 0 .. n - 1
 * with curL = n, bit for bit: the same 32-key tiles over the logical sequence, the same running-maximum recurrence, 4-interleaved fma order
 * and four partial row sums.  So a full mask leaves varhip_attn_cached_f32's bits; n == 0 writes +0 to the l x 64 outputs of (b, h); the
 * keys and values of hidden scales, and the cache beyond curL, are not read (a NaN there has no effect).
 * varhip_attn_force_waves and varhip_attn_last_waves act on this launcher as on the plain one.
 * VARHIP_EINVAL before any launch, nothing written: a NULL pointer, a size <= 0, curL > Lmax, l > curL, S1 outside [1, 16], ends not as above,
 * q, kcache or vcache not 16-byte aligned, B2 or H above 65535.  f32 only. */
/* pinned bit for bit against varhip_attn_cached_f32 on the gathered cache (tests/test_knockout_kernels_gpu.py) */
int varhip_attn_keysel_f32(const float* q, const float* kcache, const float* vcache, float* out,
                           int B2, int l, int H, int curL, int Lmax, const int32_t* ends, int S1, const int32_t* keymask,
                           varhip_stream_t stream);

/* ---- one AdaLNSelfAttn block (basic_var.py:152-159) in one call ---------------------------------------------
 * x <- x + gamma1 * proj(attn(LN(x)(1+scale1)+shift1));  x <- x + gamma2 * fc2(gelu(fc1(LN(x)(1+scale2)+shift2)))
 * issued as the seven launches ln_modulate, gemm_qkv, attn_cached, gemm_nt(RESID), ln_modulate, gemm_nt(GELU),
 * gemm_nt(RESID) with exactly their arithmetic.  ada: this block's [B2][6C] AdaLN rows (gamma1|gamma2|scale1|scale2|shift1|
 * shift2, row stride ld_ada); x2, xn, q, att, hid are workspaces ([M][C], hid [M][hidden]); the result is left in x.
 * A host that pays ~10 us per FFI call would otherwise starve the GPU at the small scales (launches of 5-20 us). */
int varhip_adaln_block_f32(float* x, float* x2, float* xn, float* q, float* att, float* hid,
                           const float* ada, int64_t ld_ada,
                           const float* qkv_w, const float* qkv_b, const float* scale_mul, float plain_scale, int l2norm,
                           const float* proj_w, const float* proj_b, const float* fc1_w, const float* fc1_b,
                           const float* fc2_w, const float* fc2_b, float* kcache, float* vcache,
                           int B2, int l, int C, int H, int hidden, int pos0, int Lmax, float eps, varhip_stream_t stream);

/* ---- classifier-free guidance + top-k/top-p + multinomial(1) -------------------------------------------
 * logits: [2B][l][V] (rows 0..B-1 conditional, B..2B-1 unconditional).  For row r=(b,t):
 *   x = (float)(1+t_cfg) * cond - (float)t_cfg * uncond                             (var.py:172-173)
 *   top_k > 0: x[x < kth_largest(x, top_k)] = -inf                                   (helpers.py:8-10)
 *   top_p > 0: ascending stable sort, softmax, cumsum (fp64 accumulate, fp32 per element), remove where
 *              cum <= (float)(1-top_p) except the largest                            (helpers.py:11-15)
 *   idx = argmax_v softmax(x)[v] / noise[r][v]    (first max)  == torch.multinomial(p, 1, generator) with
 *              noise = empty_like(p).exponential_(1, generator)                      (helpers.py:19)
 * idx_out: int64 [B*l].  masked_out (optional, may be NULL): [B*l][V] the filtered logits (what the reference leaves in place).
 * Constraint: V % 256 == 0, V <= 8192, 0 <= top_k <= V; `logits` 16-byte aligned (rows are read 16 bytes per lane; V % 256 == 0 keeps
 * every row aligned once the base is): VARHIP_EINVAL otherwise.  Any tensor start handed out by hipMalloc / torch's allocator qualifies;
 * a view at an odd element offset does not — copy it first. */
int varhip_cfg_sample_f32(const float* logits, const float* noise, int64_t* idx_out, float* masked_out,
                          int B, int l, int V, double t_cfg, int top_k, double top_p, varhip_stream_t stream);
/* test hook: 1 = every top-p cut is decided by the sequential fp64 walk (the definition); 0 (default) = by a parallel prefix sum wherever
 * that provably gives the same cut, by the walk otherwise.  Same results either way. */
int varhip_sampler_force_walk(int on);

/* The same sampler with one parameter set per image (VAR.autoregressive_infer_cfg_per_image): t_cfg [B] double, top_k [B] int32 and
 * top_p [B] double are DEVICE arrays; the workgroup of row r reads entry r / l and rounds it as varhip_cfg_sample_f32 rounds its scalars:
 * ca = (float)(1.0 + t), cb = (float)t, thr = (float)(1.0 - top_p), top-p active where top_p > 0.  Contract: for every image b, idx_out and
 * masked_out of its l rows are bit-identical to varhip_cfg_sample_f32 called on those rows alone (B = 1) with the scalars
 * (t_cfg[b], top_k[b], top_p[b]), under both settings of varhip_sampler_force_walk.  top_k_cap sizes the launch's sort buffer (the kernel's
 * results do not depend on it: ties with the k-th value beyond the buffer are handled unsorted): the largest top_k[b], or V if any
 * top_k[b] == 0; the host holds the table it uploads, so it passes the number.  An image whose top_k is outside [0, V] or needs more than
 * top_k_cap gets idx_out = -1 on its rows and leaves masked_out alone (no LDS is touched).  Constraints as varhip_cfg_sample_f32, and
 * 1 <= top_k_cap <= V: VARHIP_EINVAL otherwise. */
/* pinned against varhip_cfg_sample_f32 per image (tests/test_per_image_gpu.py) */
int varhip_cfg_sample_rows_f32(const float* logits, const float* noise, int64_t* idx_out, float* masked_out, int B, int l, int V,
                               const double* t_cfg, const int32_t* top_k, const double* top_p, int top_k_cap, varhip_stream_t stream);

/* The same sampler over G row groups with one coefficient row per image (VAR.sample_composed: weighted multi-class guidance; the reference
 * has the two-row case only, var.py:172-173).  logits: [G][B][l][V], group-major as above, the unconditional group last; coef: DEVICE fp32
 * [B][G].  With c_1 .. c_K the class rows of row r = (b, t) (K = G - 1), u its unconditional row and a = coef[b]:
 *   acc = a_1*c_1;   acc = acc + a_k*c_k  for k = 2 .. K, in this order;   x = acc - a_u*u
 * where every *, + and - is one fp32 operation rounded on its own (no fma contraction), as varhip_cfg_sample_f32's expression above: with
 * G = 2 and coef[b] = ((float)(1.0 + t), (float)t) idx_out and masked_out are bit-identical to varhip_cfg_sample_rows_f32 with t_cfg[b] = t.
 * Everything after x is that entry's: top_k [B] int32 and top_p [B] double DEVICE arrays, top_k_cap, the refused image (idx_out = -1 on
 * its rows, masked_out and guided_out left alone), both settings of varhip_sampler_force_walk.  guided_out (optional, may be NULL):
 * [B*l][V], receives x before any filtering; masked_out (optional) as above.  G < 2 or G > 9, a NULL logits / noise / idx_out / coef /
 * top_k / top_p, logits or guided_out not 16-byte aligned, and the constraints of varhip_cfg_sample_rows_f32 on B, l, V, top_k_cap:
 * VARHIP_EINVAL, nothing is written. */
/* pinned against varhip_cfg_sample_rows_f32 and a numpy float32 restatement of the mix (tests/test_compose_kernels_gpu.py) */
int varhip_mix_sample_rows_f32(const float* logits, const float* noise, int64_t* idx_out, float* masked_out, float* guided_out,
                               int B, int l, int V, int G, const float* coef, const int32_t* top_k, const double* top_p, int top_k_cap,
                               varhip_stream_t stream);

/* varhip_cfg_sample_rows_f32 with four more per-image controls (VAR.sample_controlled): a logit bias, a temperature and min-p join top-k and
 * top-p.  tau [B] and min_p [B] are DEVICE fp32 arrays; bias is a DEVICE fp32 table [R][ld_bias] (ld_bias >= V, ld_bias % 4 == 0, 16-byte
 * aligned: rows are read 16 bytes per lane), bias_row [B] a DEVICE int32 array that names each image's row of it, -1 (any negative) = none.
 * bias and bias_row may be NULL (no image has a bias; R is then not read).  Row r = (b, j), in this order:
 *   1. combine   x = ca*cond - cb*uncond from t_cfg[b], exactly as varhip_cfg_sample_rows_f32
 *   2. bias      where bias_row[b] >= 0:  x_v = x_v + bias[bias_row[b] * ld_bias + v], one fp32 add; -inf bans code v.  Where bias_row[b] < 0
 *                the stage does not run at all (a signed zero of x survives)
 *   3. temper    where tau[b] != 1:  x_v = x_v / tau[b], one correctly rounded fp32 division (no reciprocal multiply)
 *   4. top-k     as above, on the biased and tempered row
 *   5. min-p     where min_p[b] > 0:  m = the row's maximum after top-k, e_v = vm_exp(x_v - m) (include/var_math.h), x_v = -inf where
 *                e_v < min_p[b] (an fp32 compare).  The maximum has e = 1 and always survives
 *   6. top-p and the draw as above, on what remains
 * masked_out (optional) receives the row after stage 6, idx_out the drawn index.  Contracts, under both settings of
 * varhip_sampler_force_walk: with tau = 1, min_p = 0 and bias_row = -1 (or NULL) for every image, idx_out and masked_out are bit-identical
 * to varhip_cfg_sample_rows_f32 on the same operands; and for every image b, its l rows are bit-identical to the same call with B = 1 on
 * those rows and that image's parameters alone.  Refused image (idx_out = -1 on its rows, masked_out left alone, no LDS touched): top_k as
 * in varhip_cfg_sample_rows_f32; tau[b] not in (0, inf) or NaN; min_p[b] not in [0, 1] or NaN; bias_row[b] >= R.  VARHIP_EINVAL before any
 * launch, nothing written: a NULL logits / noise / idx_out / t_cfg / top_k / top_p / tau / min_p, bias_row without bias, a bias that is not
 * 16-byte aligned or whose ld_bias is below V or no multiple of 4, R < 0, and the constraints of varhip_cfg_sample_rows_f32. */
/* pinned against varhip_cfg_sample_rows_f32 on rows prepared by a numpy float32 restatement of stages 2, 3 and 5 (tests/test_controlled_kernels_gpu.py) */
int varhip_ctl_sample_rows_f32(const float* logits, const float* noise, int64_t* idx_out, float* masked_out, int B, int l, int V,
                               const double* t_cfg, const int32_t* top_k, const double* top_p, const float* tau, const float* min_p,
                               const float* bias, const int32_t* bias_row, int R, int ld_bias, int top_k_cap, varhip_stream_t stream);

/* ---- counter-based Exp(1) fill (per-image sampling) ----------------------------------------------------------------------------------------
 * out[(b*l + t)*V + v] = -vm_log(u),  u = (2n + 1) * 2^-24,  n = x >> 9,  x = word v % 4 of Philox4x32-10(counter, key) with
 *   key = (low 32 bits of seeds[b], high 32 bits of seeds[b]),  counter = (v / 4, t, scale, draw)
 * (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85: Random123's philox4x32_10).  The value is a function of
 * (seed, scale, t, v, draw) alone: not of B, of the image's position in the batch, or of what was drawn before.  draw: 0 = the multinomial
 * fill (the noise of varhip_cfg_sample*_f32), 1 = the gumbel fill of more_smooth (the noise of varhip_gumbel_softmax_f32), 2 and 3 = the fresh
 * values of varhip_exp1_posterior_f32 below (the losers' E_v, and at v = 0 the minimum T).  u is exact in
 * fp32 and lies in [2^-24, 1 - 2^-24]; vm_log (include/var_math.h) consists of correctly rounded operations only, so the kernel and the
 * host twin give the same bits.  This is the project's own stream, not torch's.  seeds: DEVICE int64 [B] (the host twin: host pointers);
 * out 16-byte aligned (the kernel stores 16 bytes per lane).  V % 4 != 0, B or l < 1, scale or draw < 0, a misaligned out: VARHIP_EINVAL. */
/* pinned against its host twin below (tests/test_per_image_gpu.py) */
int varhip_exp1_philox_f32(const int64_t* seeds, int B, int l, int V, int scale, int draw, float* out, varhip_stream_t stream);
/* the host twin: plain host code (usable without a GPU), same arguments with host pointers, no alignment constraint */
/* pinned against a numpy Philox4x32-10 (tests/test_per_image_cpu.py) */
int varhip_exp1_philox_host_f32(const int64_t* seeds, int B, int l, int V, int scale, int draw, float* out);
/* one Philox4x32-10 block on the host (known-answer tests of the integer stage against the published vectors) */
/* pinned against the Random123 known answers (tests/test_per_image_cpu.py) */
int varhip_philox4x32_host(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
/* the fill's transform alone on the host: out[i] = -vm_log((2 (bits[i] >> 9) + 1) * 2^-24)  (exhaustive tests over the 2^23 values of n) */
int varhip_exp1_from_bits_host_f32(const uint32_t* bits, int64_t n, float* out);

/* ---- posterior Exp(1) noise given the drawn token (VAR.abduct_noise / VAR.counterfactual) ----------------------------------------------------
 * The noise under which varhip_cfg_sample_rows_f32, without top-k / top-p, draws the GIVEN token g from the given logits, sampled from the
 * law of the Exp(1) noise conditioned on that outcome (the Gumbel-max posterior in its exponential-race form).
 * logits: [2B][l][V] as the sampler reads them (conditional rows first); t_cfg: DEVICE double [B]; gt: int64, the token of row (b, t) at
 * gt[b * ld_gt + t]; seeds: DEVICE int64 [B]; every output of row (b, t) is addressed at row b * ld_out + t (ld_gt, ld_out >= l: a scale
 * reads and writes its slice of (B, L) tensors).  Row (b, t), one 256-thread workgroup:
 *   x_v = ca*cond_v - cb*uncond_v, ca = (float)(1.0 + t_cfg[b]), cb = (float)t_cfg[b]      the sampler's combine, one piece of code
 *   m = max x,  ev_v = vm_exp(x_v - m),  S = the sampler's canonical W256 sum of ev,  p_v = ev_v / S      the sampler's stage (4) values
 *   E_v = the Exp(1) stream's value at (seeds[b], scale, t, v, draw 2),  T = its value at (seeds[b], scale, t, 0, draw 3)
 *   noise_g = max(fl(T * p_g), FLT_MIN);   r_g = p_g / noise_g
 *   noise_v (v != g) = the smallest float n >= fl(fl(T * p_v) + E_v) with (ev_v / S) / n < r_g strictly in fp32 — the sampler's own score
 *             expression; reached from max(that candidate, pred(fl(p_v / r_g))) by five conditional one-ulp steps, no data-dependent loop
 *   logp = (x_g - m) - vm_log(S),  flag = 0
 * A row whose g lies outside [0, V), that holds a NaN, whose p_g == 0 or whose r_g is not finite and positive is flagged and not repaired:
 * flag = 1, logp = -inf, noise_v = E_v for every v (the prior).  On every unflagged row varhip_cfg_sample_rows_f32 with top_k = 0,
 * top_p = 0 and this noise returns g, under both settings of varhip_sampler_force_walk.  V % 4 != 0, V > 8192, B or l < 1, scale < 0,
 * ld_gt or ld_out < l, a NULL operand, logits or noise_out not 16-byte aligned: VARHIP_EINVAL, nothing is written. */
/* pinned against its host twin below and the sampler's replay (tests/test_abduct_kernels_gpu.py) */
int varhip_exp1_posterior_f32(const float* logits, const double* t_cfg, const int64_t* gt, int64_t ld_gt, const int64_t* seeds, int B, int l,
                              int V, int scale, float* noise_out, float* logp_out, int32_t* flag_out, int64_t ld_out, varhip_stream_t stream);
/* the host twin: plain host code (usable without a GPU), same arguments with host pointers, no alignment constraint; the kernel's bits */
/* pinned against a numpy restatement, the oracle's sampler and the Exp(1) law (tests/test_abduct_cpu.py) */
int varhip_exp1_posterior_host_f32(const float* logits, const double* t_cfg, const int64_t* gt, int64_t ld_gt, const int64_t* seeds, int B, int l,
                                   int V, int scale, float* noise_out, float* logp_out, int32_t* flag_out, int64_t ld_out);

/* ---- scored sampling (VAR.autoregressive_infer_cfg_scored, VAR.sample_best_of) -----------------------------------------------------------
 * What the sampler's operands say about the token it drew, one wave per token row r = b * l + j, launched right behind varhip_cfg_sample*_f32
 * of a scale.  logits: [2B][l][V] as the sampler reads them (conditional rows first); masked: [B*l][V], the sampler's masked_out; idx: [B*l],
 * its idx_out.  Guidance: the scalar t_cfg, or, where t_rows != NULL, the DEVICE array t_rows[B] (t_cfg is then not read), rounded as the
 * samplers round it: ca = (float)(1.0 + t), cb = (float)t, z = ca * cond - cb * uncond with each product and the difference rounded to fp32.
 * Every output is addressed out[b * ld_out + j] (ld_out >= l: a scale writes its slice of a (B, L) tensor; nothing else is written):
 *   lp_cond   fp32   log_softmax(cond)[idx]: varhip_token_loglik_f32 without guidance on the same row, bit for bit (one piece of device code)
 *   lp_guided fp32   log_softmax(z)[idx]: varhip_token_loglik_f32 with (ca, cb) on the same rows, bit for bit
 *   lp_drawn  fp32   log_softmax(masked)[idx]: the distribution the token was drawn from; a -inf entry adds 0 to the sum
 *   kept      int32  the number of entries of the masked row that are not -inf
 *   entropy   fp32   -sum_v p_v log p_v of the guided row in nats, 0 * log 0 = 0: (float)((0 - A) / (double)s), A = sum_v (double)e_v * (double)lp_v
 *                    over the elements with e_v > 0, where m = max z, e_v = vm_exp(z_v - m), s = the row's fp32 sum of exponentials (the one lp_guided
 *                    uses) and lp_v = (z_v - m) - vm_log(s).  A is accumulated in float64 in ONE order that depends on V alone, the order of
 *                    varhip_token_eval_f32's `smooth` sum: lane i of 64 adds its elements j * 256 + 4 * i + c in ascending (j, c) order, the
 *                    lanes by the xor butterfly 32, 16, 8, 4, 2, 1.  Rounded once to fp32.  A guided row holding a NaN: NaN.
 * An idx outside [0, V) (the -1 varhip_cfg_sample_rows_f32 writes for a refused image) is never dereferenced: the three log-probabilities of
 * the row are NaN, kept and entropy are still the row's own.  On a row holding a NaN the log-probabilities are what varhip_token_loglik_f32
 * gives there.  Constraints as the samplers': V % 256 == 0, V <= 8192, logits and masked 16-byte aligned; a NULL operand (t_rows excepted),
 * B or l < 1 or ld_out < l: VARHIP_EINVAL. */
/* pinned against its host twin, varhip_token_loglik_f32 and float64 (tests/test_sample_stats_gpu.py) */
int varhip_sample_stats_f32(const float* logits, const float* masked, const int64_t* idx, int B, int l, int V, double t_cfg,
                            const double* t_rows, float* lp_cond, float* lp_guided, float* lp_drawn, int32_t* kept, float* entropy,
                            int64_t ld_out, varhip_stream_t stream);
/* the host twin: plain host code (usable without a GPU), same arguments with host pointers, no alignment constraint.  The same operations in
 * the same order (vm_exp / vm_log consist of correctly rounded operations only): the kernel's bits. */
/* pinned against float64 (tests/test_sample_stats_cpu.py) */
int varhip_sample_stats_host_f32(const float* logits, const float* masked, const int64_t* idx, int B, int l, int V, double t_cfg,
                                 const double* t_rows, float* lp_cond, float* lp_guided, float* lp_drawn, int32_t* kept, float* entropy,
                                 int64_t ld_out);

/* ---- lossless token coding (VAR.compress / VAR.decompress) -------------------------------------------------------------------------------
 * The model as the probability source of a range coder.  A decoder must rebuild every table its encoder used to the last bit, on another
 * batch and in another call order, so the table is defined by exact integer operations on the row's exponentials:
 * THE TABLE.  Row r = b * l + j of a scale's [2B][l][V] logits (conditional rows first) becomes F[V], positive integers that sum to exactly
 * 2^PB, PB = VARCODEC_PB.  With the guidance t (the scalar t_cfg, or the DEVICE array t_rows[B] where t_rows != NULL):
 *   z_v = ca * cond_v - cb * uncond_v,  ca = (float)(1.0 + t), cb = (float)t, each product and the difference rounded to fp32 (as
 *         varhip_cfg_sample_f32 and varhip_token_loglik_f32 form it)
 *   m   = max_v z_v;  e_v = vm_exp(z_v - m)  (include/var_math.h; a -inf entry gives e_v = 0, the maximum gives e_v = 1)
 *   i_v = (uint64)floor((double)e_v * 2^32)                              exact in double, i_v <= 2^32
 *   I   = sum_v i_v                                                      an exact integer sum (< 2^46 for V <= 8192): order does not matter
 *   K   = 2^PB - V;  q_v = (i_v * K) / I                                 unsigned 64-bit integer division, the product is below 2^57
 *   D   = K - sum_v q_v                                                  0 <= D < V
 *   F_v = 1 + q_v, and the lowest index v* with z_v == m also takes D;   C_v = sum_{u < v} F_u, the exclusive prefix in index order
 * Nothing above depends on who computes it or in what order: any implementation of these lines gives the same F.  A row that holds a NaN, or
 * whose maximum is +inf or -inf (no finite entry), is REFUSED: nothing is coded from it.
 * Addressing: gt, pair_out and flag_out share the row stride ld >= l (a scale's slice of (B, L) tensors): gt[b * ld + j], flag_out[b * ld + j],
 * pair_out[2 * (b * ld + j) + {0, 1}].  Outputs:
 *   cum_out  (may be NULL) uint32 [B*l][V], dense: the INCLUSIVE cumulative table C_v + F_v (its last entry is 2^PB); a refused row is all 0,
 *            a table in which no slot has an owner
 *   pair_out (NULL exactly when gt is NULL) (C_g, F_g) of the row's token g = gt[b * ld + j]; (0, 0) on a refused row or a g outside [0, V)
 *   flag_out int32, written for every row: 0, 1 = the row was refused, 2 = g lies outside [0, V) (never dereferenced)
 * cum_out and pair_out must not both be NULL.  Constraints as the samplers': V % 256 == 0, V <= 8192, logits (and cum_out) 16-byte aligned,
 * B, l >= 1, ld >= l; anything else: VARHIP_EINVAL before any launch.  One wave per row, four rows per workgroup. */
#define VARCODEC_PB 24
/* pinned against its host twin bit for bit (tests/test_codec_kernels_gpu.py) */
int varhip_code_table_f32(const float* logits, int B, int l, int V, double t_cfg, const double* t_rows, const int64_t* gt, int64_t ld,
                          uint32_t* cum_out, uint32_t* pair_out, int32_t* flag_out, varhip_stream_t stream);
/* the host twin: plain host code, host pointers (t_rows too), no alignment constraint; the same integers by the definition above */
/* pinned against the Python-integer restatement of the definition in tests/codecref.py (tests/test_codec_cpu.py) */
int varhip_code_table_host_f32(const float* logits, int B, int l, int V, double t_cfg, const double* t_rows, const int64_t* gt, int64_t ld,
                               uint32_t* cum_out, uint32_t* pair_out, int32_t* flag_out);
/* THE CODER: rANS with a 64-bit state x in [2^31, 2^63) and 32-bit words.
 *   encoding (C, F):  if x >= ((2^31 >> PB) << 32) * F: emit the low 32 bits of x, x >>= 32.  Then x = ((x / F) << PB) + x % F + C.
 *   Symbols are encoded in REVERSE token order from x = 2^31.  The stream: the final state as two words (high word first), then the emitted
 *   words in reverse order of emission, so the decoder reads forward.
 *   decoding:  slot = x & (2^PB - 1); s = the symbol with C_s <= slot < C_s + F_s; x = F_s * (x >> PB) + slot - C_s; if x < 2^31:
 *   x = x << 32 | next word.  After the last token of a complete stream x == 2^31 and every word has been read: the integrity check.
 * varhip_rans_encode_host: pairs = n (C, F) pairs in token order; words_out[cap] receives the stream, *nwords_out its length (<= n + 2).
 * n < 0, a NULL pointer, a pair with F == 0 or C + F > 2^PB, or a stream longer than cap: VARHIP_EINVAL. */
int varhip_rans_encode_host(const uint32_t* pairs, int64_t n, uint32_t* words_out, int64_t cap, int64_t* nwords_out);
/* varhip_rans_decode_u32: the l tokens of one scale for each of B images from cum = the scale's cum_out [B*l][V]; one wave per image, serial
 * over its tokens, the 64 lanes searching a row in two dependent rounds (lane i reads entry (V / 64) * i + V / 64 - 1, a ballot picks the
 * segment, the lanes then read inside it).  Image b's stream is words[word_off[b] .. word_off[b] + nwords[b]) (DEVICE arrays), words_total
 * the length of `words`.  state: uint32 [B][4] = (x low, x high, words consumed, started), carried between the scales of a call: all zero
 * before the first scale (the kernel then reads the stream's two state words), the end check reads it after the last.  err_out int32 [B],
 * zero before the first scale, sticky: 1 = a read past the image's words, 2 = a slot no symbol owns (a refused row's table), 3 = the image's
 * word range does not lie inside `words`.  From the token at which an error is found on, the image's tokens are -1 (idx_out int64 [B*l]), in
 * this and every later scale; a token whose symbol was found before a refill ran past the end is still written.  Every read of `words` is
 * checked against the image's nwords and every loop is bounded by l and V: never by data.  V % 256 == 0, V <= 8192, B, l >= 1, words_total
 * >= 0, no NULL pointer; anything else: VARHIP_EINVAL. */
/* pinned against its host twin (tests/test_codec_kernels_gpu.py) */
int varhip_rans_decode_u32(const uint32_t* cum, int l, int V, const uint32_t* words, int64_t words_total, const int64_t* word_off,
                           const int64_t* nwords, uint32_t* state, int64_t* idx_out, int32_t* err_out, int B, varhip_stream_t stream);
/* the host twin: the same search and the same state transitions on host pointers */
/* pinned against the Python-integer coder of tests/codecref.py (tests/test_codec_cpu.py) */
int varhip_rans_decode_host(const uint32_t* cum, int l, int V, const uint32_t* words, int64_t words_total, const int64_t* word_off,
                            const int64_t* nwords, uint32_t* state, int64_t* idx_out, int32_t* err_out, int B);

/* ---- multi-scale quantizer step ---------------------------------------------------------------------------
 * Feature maps are kept channels-last: f_hat[B][P][P][Cv].
 * (1) h = codebook[idx] as [B][pn][pn][Cv]                                          (var.py:177,182; quant.py:39)
 * (2) up = bicubic(h -> PxP) via 4-tap tables (tap_idx/tap_w: [P][4], same table for rows and columns; NULL when pn==P)
 *                                                                                    (quant.py:190, F.interpolate 'bicubic')
 * (3) f_hat += (1-ratio)*up + ratio*(conv3x3(up; phi_w[Cv][3][3][Cv]) + phi_b)      (quant.py:199-206, :191)
 * `up` is caller-provided scratch [B][P][P][Cv]. */
int varhip_quant_accum_f32(const int64_t* idx, const float* codebook, const int32_t* tap_idx, const float* tap_w,
                           const float* phi_w, const float* phi_b, float ratio,
                           float* up, float* f_hat, int B, int pn, int P, int Cv, varhip_stream_t stream);

/* Same step with the scale's embeddings given directly, h: [B][pn*pn][Cv] (more_smooth: gumbel-softmax @ codebook, var.py:178-182) */
int varhip_quant_accum_h_f32(const float* h, const int32_t* tap_idx, const float* tap_w,
                             const float* phi_w, const float* phi_b, float ratio,
                             float* up, float* f_hat, int B, int pn, int P, int Cv, varhip_stream_t stream);

/* y[r][:] = softmax((x[r][:] * mul + (-ln noise[r][:])) / tau)   — gumbel_softmax_with_rng(logits.mul(1+ratio), tau, hard=False, rng)
 * (helpers.py:22-36, var.py:179-180); x are the top-k/top-p filtered CFG logits (-inf entries give probability 0). V % 256 == 0. */
int varhip_gumbel_softmax_f32(const float* x, const float* noise, float* y, int64_t rows, int V, float mul, float tau, varhip_stream_t stream);

/* (4) next-scale input: pooled = adaptive_avg_pool(f_hat -> pq x pq)  (quant.py:192, F.interpolate 'area');
 *     x[b][t][:] = x[b+B][t][:] = word_w[C][Cv] . pooled[b][t][:] + word_b + lvl_pos[t][:]     (var.py:185-187)
 * lvl_pos must already point at row cur_L.  pooled: caller-provided [B][pq*pq][Cv] buffer (intermediate; kept for inspection). */
int varhip_next_map_f32(const float* f_hat, const float* word_w, const float* word_b, const float* lvl_pos,
                        float* x_out, float* pooled, int B, int P, int pq, int C, int Cv, varhip_stream_t stream);
/* testing (a host global, no launch): the kernel route of the latest call of this process among the quantizer steps (varhip_quant_accum_f32,
 * _h_f32, varhip_quant_residual_f32, the _edit_ forms: 1 = the LDS-staged Phi kernel, 2 = the plain one), the word embedding
 * (varhip_next_map_f32, varhip_word_embed_f32: 4 = the Cv == 32 kernel, 8 = the generic one) and the nearest-code lookups (16 = the MFMA kernel,
 * 32 = the generic one); 0 before any such call, unchanged by a call that returned VARHIP_EINVAL.  Every route computes the same bits. */
int varhip_quant_last_route(void);

/* lvl_pos[t][:] = lvl_embed[lvl[t]][:] + pos[t][:]     (var.py:153) */
int varhip_lvl_pos_f32(const float* lvl_embed, const int64_t* lvl, const float* pos, float* out, int L, int C, varhip_stream_t stream);

/* prologue (var.py:151,154): cond[b2][:] = class_emb[b2 < B ? label[b2] : num_classes][:];
 * x[b2][t][:] = (cond[b2][:] + pos_start[t][:]) + lvl_pos[t][:],  t < first_l */
int varhip_first_map_f32(const float* class_emb, const int64_t* labels, int num_classes, const float* pos_start,
                         const float* lvl_pos, float* cond, float* x_out, int B, int C, int first_l, varhip_stream_t stream);

/* ---- VQVAE decoder (channels-last) ----------------------------------------------------------------------
 * 3x3 convolution, stride 1, zero padding 1 (cross-correlation), w packed [Cout][3][3][Cin]:
 *   out[b][y][x][co] = sum_{ky,kx,ci} in[b][y+ky-1][x+kx-1][ci] * w[co][ky][kx][ci] + bias[co]  (+ resid[b][y][x][co])
 *   up2 != 0: `in` is [B][H/2][W/2][Cin] and is read through a nearest-neighbour 2x upsampling
 *             (basic_vae.py:27-28 Upsample2x: F.interpolate(scale 2,'nearest') then conv)
 *   out_mode 0: out is [B][H][W][Cout];  out_mode 1: out is [B][Cout][H][W] and holds (clamp(v,-1,1)+1)*0.5
 *             (vqvae.py:63 clamp_ and var.py:190 add_(1).mul_(0.5) fused into the last conv);
 *   out_mode 2: [B][Cout][H][W] holding clamp(v,-1,1) only (VQVAE.fhat_to_img's own contract)
 *   out_mode 3: [B][Cout][H][W] holding v itself (VQVAE.forward, vqvae.py:59: the decoder's output without a clamp)
 * replaces every Conv2d(k=3) of basic_vae.py (ResnetBlock :48,:51; conv_in :180; conv_out :208; Upsample2x :25)
 * and vqvae.py:49 post_quant_conv.   Constraints: Cin % 32 == 0 (a K tile of the implicit GEMM lies inside one tap); the input
 * samples one 128-pixel tile can touch (one sample when H*W >= 128) plus one row must span < 2 GiB and the packed weights < 4 GiB
 * (buffer-descriptor window / 32-bit offsets of the DMA requests; VARHIP_EINVAL otherwise).  The batch itself may exceed 4 GiB.
 * Summation order (arithmetic contract of every 3x3 convolution here): one fma chain per output over 32-channel chunks
 * (outermost), then the taps (ky, kx), then the channels of the chunk. */
int varhip_conv3x3_nhwc_f32(const float* in, const float* w, const float* bias, const float* resid, float* out,
                            int B, int H, int W, int Cin, int Cout, int up2, int out_mode, varhip_stream_t stream);

/* Upsample2x (basic_vae.py:27-28: nearest 2x, then conv3x3) as four 2x2 convolutions on the LOW-resolution map, one per output
 * parity (py,px): the 3x3 taps that read the same source pixel through the upsampling are pre-summed, 2.25x fewer MACs.
 *   varhip_upconv_pack_f32 : w [Cout][3][3][Cin] -> w_phase [4][Cout][2][2][Cin]   (one-time, per weight)
 *   varhip_upconv_phase_f32: in [B][H/2][W/2][Cin] -> out [B][H][W][Cout], bias added
 * Mathematically equal to varhip_conv3x3_nhwc_f32(up2=1); rounding differs at the 1e-7 level (decoder only: pixels, not tokens). */
int varhip_upconv_pack_f32(const float* w, float* w_phase, int Cin, int Cout, varhip_stream_t stream);
int varhip_upconv_phase_f32(const float* in, const float* w_phase, const float* bias, float* out,
                            int B, int H, int W, int Cin, int Cout, varhip_stream_t stream);
/* ... and with the GroupNorm partials of its result (see varhip_conv3x3_gn_nhwc_f32): block blk = phase * ((H/2)*(W/2)/128) + t
 * covers low-resolution pixels [128 t, 128 t + 128) of that phase */
int varhip_upconv_phase_gn_f32(const float* in, const float* w_phase, const float* bias, float* out, double* gn_part,
                               int B, int H, int W, int Cin, int Cout, varhip_stream_t stream);

/* GroupNorm statistics: stats[b][g] = {mean, rstd} over (HW, C/G) with biased variance (basic_vae.py:18-19, eps 1e-6).
 * scratch: caller-provided, at least varhip_gn_scratch_elems(B,HW,C,G) doubles.  C % 4 == 0, C <= 1024 (fp32; the 16-bit forms: C % 8 == 0,
 * C <= 2048), G divides C, any HW.  A null x, stats, scratch (gamma, beta, out for the apply) is VARHIP_EINVAL. */
int64_t varhip_gn_scratch_elems(int B, int HW, int C, int G);
int varhip_gn_stats_f32(const float* x, float* stats, double* scratch, int B, int HW, int C, int G, float eps, varhip_stream_t stream);
/* out = ((x - mean) * rstd) * gamma[c] + beta[c], then SiLU if silu != 0   (basic_vae.py:58,59,74,225) */
int varhip_gn_apply_f32(const float* x, const float* stats, const float* gamma, const float* beta, float* out,
                        int B, int HW, int C, int G, int silu, varhip_stream_t stream);

/* the decoder's tail in one pass (basic_vae.py:224-226 norm_out -> swish -> conv_out, the callers' clamp vqvae.py:63 and (x + 1) / 2 var.py:190):
 * out = clamp(conv3x3(SiLU(GroupNorm(x))) + bias, -1, 1) as fp32 NCHW (out_mode 2) or de-normalised to [0, 1] (out_mode 1); stats [B][G][2] = (mean, rstd).
 * out_mode 3: no clamp (vqvae.py:59, VQVAE.forward): the value modes 1 and 2 clamp, stored as it is.
 * Bit-identical to varhip_gn_apply_f32 (silu = 1) followed by varhip_conv3x3_nhwc_f32 (same out_mode): same operations per element, same
 * chunk / tap / channel summation order.  Shapes it does not take (H % 8, W % 32, Cin % 32, Cout > 4): VARHIP_EINVAL. */
int varhip_gn_silu_conv_out_f32(const float* x, const float* stats, const float* gamma, const float* beta, const float* w, const float* bias,
                                float* out, int B, int H, int W, int Cin, int Cout, int G, int out_mode, varhip_stream_t stream);

/* out[r][:] = softmax(x[r][:] * scale), rows of length n   (basic_vae.py:83-84: bmm(...).mul_(w_ratio); softmax(dim=2)) */
int varhip_softmax_rows_f32(const float* x, float* out, int64_t rows, int n, float scale, varhip_stream_t stream);

/* [B][C][H][W] <-> [B][H][W][C] copies for the API edge (f_hat is NCHW in the reference's API) */
int varhip_nchw_to_nhwc_f32(const float* in, float* out, int B, int C, int HW, varhip_stream_t stream);
int varhip_nhwc_to_nchw_f32(const float* in, float* out, int B, int C, int HW, varhip_stream_t stream);

/* ---- encode side and teacher forcing ("next" rows of SURVEY.md §8f: image -> tokens -> teacher-forced logits) -----------------
 * Downsample2x of the encoder (basic_vae.py:31-37): F.pad(x,(0,1,0,1)) + Conv2d(k=3, stride=2): in [B][2H][2W][Cin] -> out [B][H][W][Cout] */
/* The same convolution (out_mode 0) that also leaves GroupNorm partial sums of its result: gn_part[b][blk][co][2] (doubles) =
 * (sum, sum of squares) over the blk-th block of 128 consecutive pixels of sample b, so the GroupNorm that follows
 * (basic_vae.py:18-19 inside ResnetBlock / AttnBlock / norm_out) needs no statistics pass over the tensor.
 * varhip_conv_gn_blocks(H, W, Cout, phase) = blocks per sample, or 0 when unsupported (needs H*W % 128 == 0, Cout % 32 == 0;
 * phase != 0 describes varhip_upconv_phase_gn_f32 below: 4 * ((H/2)*(W/2) / 128) blocks, phase-major).
 * varhip_gn_stats_part_f32 turns the partials into the (mean, rstd) pairs varhip_gn_apply_f32 takes (blocks in order, channels of
 * a group in order, fp64). */
int varhip_conv_gn_blocks(int H, int W, int Cout, int phase);
int varhip_conv3x3_gn_nhwc_f32(const float* in, const float* w, const float* bias, const float* resid, float* out, double* gn_part,
                               int B, int H, int W, int Cin, int Cout, int up2, varhip_stream_t stream);
int varhip_gn_stats_part_f32(const double* gn_part, float* stats, int B, int nblk, int HW, int C, int G, float eps, varhip_stream_t stream);
/* The stride-1 3x3 convolution (padding 1, NHWC, out_mode 0) as fused Winograd F(2x2,3x3): in [B][H][W][Cin], u = G g G^T of the kernel
 * [16][Cin/16][Cout][16] (xi = 4 i + j of the 4x4 transform, then input-channel tile, output channel, input channel in the tile; made once
 * per weight, DecoderEngine.refresh), out [B][H][W][Cout] = conv + bias (+ resid).  Mathematically varhip_conv3x3_nhwc_f32 (up2 0); the
 * rounding differs (measured 0.32-0.34x the direct kernel's max error against float64).  gn_part (may be NULL): as
 * varhip_conv3x3_gn_nhwc_f32 with the same block count H*W/128, but block 2 t + h is the 8-row half h (0 upper, 1 lower) of the t-th
 * 16 x 16 patch of the image in row-major patch order.  Needs H % 16 == 0, W % 16 == 0, Cin % 32 == 0, Cout % 32 == 0, 16-byte
 * aligned pointers; else VARHIP_EINVAL.  Results do not depend on B or on the image's position in the batch. */
/* pinned against float64 and the direct conv (tests/test_winograd_gpu.py) */
int varhip_conv3x3_wino_nhwc_f32(const float* in, const float* u, const float* bias, const float* resid, float* out, double* gn_part,
                                 int B, int H, int W, int Cin, int Cout, varhip_stream_t stream);
/* Upsample2x (nearest 2x, then conv3x3, padding 1) as position-sparse Winograd F(2x2,3x3) on the LOW-resolution map: in [B][H/2][W/2][Cin],
 * w_phase the pre-summed phase kernels of varhip_upconv_pack_f32 (no table of its own), out [B][H][W][Cout] = conv + bias.
 * Every 2x2 output tile at even coordinates sees a window whose rows and columns repeat (a, b, b, c), so row 2 and column 2 of B^T d B
 * vanish: 9 multiplies per tile and (ci, co) instead of 16; the rows 0, 1, 3 of G g G^T are sums of phase taps.
 * Mathematically varhip_upconv_phase_f32 and varhip_conv3x3_nhwc_f32 (up2 1); the rounding differs.  gn_part (may be NULL): H*W/128 blocks
 * per sample, as many as varhip_upconv_phase_gn_f32 writes, but block 2 t + h is the 8-row half h of the t-th 16 x 16 output patch.
 * Needs H % 16 == 0, W % 16 == 0, Cin % 32 == 0, Cout % 32 == 0, 16-byte aligned pointers; else VARHIP_EINVAL.  Results do not depend on
 * B or on the image's position in the batch.  varhip_upconv_phase_f32 / varhip_upconv_phase_gn_f32 run this kernel for such shapes while
 * the exported int vh_g_upconv_wino is non-zero (0 by default; var_amd.hip.upconv_winograd, set by the fp32 decoder around its launches). */
/* pinned against float64 and the phase form (tests/test_winograd_up_gpu.py) */
int varhip_conv3x3_wino_up_nhwc_f32(const float* in, const float* w_phase, const float* bias, float* out, double* gn_part,
                                    int B, int H, int W, int Cin, int Cout, varhip_stream_t stream);
int varhip_conv3x3_s2_nhwc_f32(const float* in, const float* w, const float* bias, float* out,
                               int B, int H, int W, int Cin, int Cout, varhip_stream_t stream);
/* The 16-bit Downsample2x of the encoder (basic_vae.py:31-37: F.pad(0, 1, 0, 1) + 3x3 conv of stride 2): the index rule of
 * varhip_conv3x3_s2_nhwc_f32 on 16-bit operands (in [B][2H][2W][Cin], w [Cout][3][3][Cin]), fp32 accumulation on the 16-bit MFMA, + bias
 * (fp32), rounded once to the storage type: out [B][H][W][Cout].  Needs Cin % 32 == 0, Cout % 16 == 0, 16-byte aligned in / w, 8-byte
 * aligned out; else VARHIP_EINVAL.  "f16" / "bf16": the two storage types (elem16.h). */
/* pinned against a CPU twin (tests/test_generative_gpu.py) */
int varhip_conv3x3_s2_nhwc_f16(const void* in, const void* w, const float* bias, void* out, int B, int H, int W, int Cin, int Cout,
                               varhip_stream_t stream);
int varhip_conv3x3_s2_nhwc_bf16(const void* in, const void* w, const float* bias, void* out, int B, int H, int W, int Cin, int Cout,
                                varhip_stream_t stream);
/* image [B][C][HW] -> [B][HW][Cpad] with zero channels C..Cpad-1 (conv kernels need Cin % 32 == 0; zero channels add exact zeros) */
int varhip_nchw_to_nhwc_pad_f32(const float* in, float* out, int B, int C, int HW, int Cpad, varhip_stream_t stream);
/* pooled[b][t][:] = mean of f[b] over the adaptive window of output cell t   (F.interpolate(mode='area'), quant.py:150,183) */
int varhip_area_pool_f32(const float* f, float* pooled, int B, int P, int pq, int Cv, varhip_stream_t stream);
/* x[b][t][:] = x[b+B][t][:] = word_w . pooled[b][t][:] + word_b + lvl_pos[t][:]   (var.py:186-187, 206-207); x_out holds 2*B*lq rows */
int varhip_word_embed_f32(const float* pooled, const float* word_w, const float* word_b, const float* lvl_pos,
                          float* x_out, int B, int lq, int C, int Cv, varhip_stream_t stream);
/* one scale of VectorQuantizer2.f_to_idxBl_or_fhat (quant.py:159-163): as varhip_quant_accum_f32, and f_rest -= the same h */
int varhip_quant_residual_f32(const int64_t* idx, const float* codebook, const int32_t* tap_idx, const float* tap_w,
                              const float* phi_w, const float* phi_b, float ratio, float* up, float* f_hat, float* f_rest,
                              int B, int pn, int P, int Cv, varhip_stream_t stream);

/* out[i] = keep[i] ? gt[i] : sampled[i]   — VAR.inpainting's torch.where(mask, gt_tokens, sampled_tokens) (var.py:312-328, fork) */
int varhip_token_select_i64(const uint8_t* keep, const int64_t* gt, const int64_t* sampled, int64_t* out, int64_t n, varhip_stream_t stream);

/* ---- VAR.smooth_sampling (fork, var.py:367-572) ----------------------------------------------------------
 * Neighbour table of the codebook (var.py:459-462: cdist + argsort + [:, :n]): nbr_idx[v][c] = the c-th nearest code of v
 * (c = 0 is v itself), nbr_dist[v][c] its L2 distance; ascending distance, ties by index.  Distances are the direct form
 * sqrt(sum (a-b)^2), one fma chain over the channels (the reference's BLAS-based cdist differs from it by rounding only).
 * codebook: [V][D], V <= 8192, 1 <= n <= V. */
int varhip_neighbor_table_f32(const float* codebook, int V, int D, int n, int32_t* nbr_idx, float* nbr_dist, varhip_stream_t stream);
/* One scale's selection (var.py:482-537).  logits: [2B][l][V] (CFG pair), gt: [B*l] ground-truth tokens of the scale.
 *   lp = log_softmax((1+t)*cond - t*uncond);  candidates = nbr_idx[gt][0..n);
 *   use_thr == 0: the first cand_count candidates are valid;  use_thr != 0: those with dist <= d0 + (thr - d0)*ratio;
 *   idx_out = the valid candidate with the largest lp (first on ties; none valid -> candidate 0, maxval -inf),
 *   maxval_out = its lp, distlp_out = log_softmax(-nbr_dist[gt][0..n))[winner];  cfg_out (nullable): the combined logits [B*l][V]. */
int varhip_smooth_select_f32(const float* logits, const int64_t* gt, const int32_t* nbr_idx, const float* nbr_dist, int n,
                             int cand_count, int use_thr, float thr, float ratio, int B, int l, int V, double t_cfg,
                             int64_t* idx_out, float* maxval_out, float* distlp_out, float* cfg_out, varhip_stream_t stream);

/* ---- teacher-forced class scoring (fork eval_prob.py:441-463 bayesian mode, var_analysis.py:322-349 guided likelihood) ----------------
 * log_softmax(logits).gather(gt) of one scale of one pass, without the (rows, V) log_softmax tensor.  logits: the head's fp32 output of the
 * pass, rows image-major, then class, then token: row (i * classes + c) * l + t; with_uncond != 0: the images' unconditional rows follow,
 * row (images * classes + i) * l + t, and z = ca * cond - cb * uncond (each product and the difference rounded to fp32; the caller passes
 * ca = fl32(1 + t), cb = t, t = fl32(fl32(cfg) * fl32(si / (S-1)))), else z = logits.  gt: the pass's tokens at the scale's offset,
 * gt[i * ld_gt + t] (a token outside [0, V) scores NaN and is never read); out[i * ld_out_img + c * ld_out_cls + t] = (z_gt - max z) - log(sum exp(z - max z)).
 * Not bit-identical to torch.log_softmax (another summation order): within a few ulps of the log-sum-exp of a float64 evaluation. */
/* pinned against float64 log_softmax (tests/test_likelihood_gpu.py) */
int varhip_token_loglik_f32(const float* logits, const int64_t* gt, int64_t ld_gt, int images, int classes, int l, int V,
                            int with_uncond, float ca, float cb, float* out, int64_t ld_out_img, int64_t ld_out_cls, varhip_stream_t stream);

/* ---- the fork's other class scores (eval_prob.py:37-92 + 518-553 smooth_bayesian, :389-393 + 559-577 fast_neighbor_bayesian,
 * var_analysis.py:252-258 + 468-500 l2_dist) -------------------------------------------------------------------------------------------
 * The codebook distance table: out[v * V + u] = sqrt(sum_c (cb[v][c] - cb[u][c])^2) with the arithmetic of varhip_neighbor_table_f32 (one fma
 * chain over the channels in channel order, then sqrt): every entry equals that table's distance for the same pair bit for bit; the table is
 * exactly symmetric with a zero diagonal.  codebook: [V][D], 1 <= V <= 65535; out: [V][V]. */
/* pinned against varhip_neighbor_table_f32 (tests/test_token_scores_gpu.py) */
int varhip_code_dist_f32(const float* codebook, int V, int D, float* out, varhip_stream_t stream);
/* One scale of one pass of teacher-forced scoring: the pass layout, gt / out addressing and CFG combine of varhip_token_loglik_f32, and
 * p = softmax(z) per row, codes ordered by z descending with ties by ascending code index:
 *   mode 1 (group_smoothed, param = group G >= 1): r = rank of gt, lo = r - r % G, hi = min(lo + G, V):
 *          out = log(sum_{rank in [lo, hi)} p / (hi - lo) + 1e-10)                                                  (eval_prob.py:37-92)
 *   mode 2 (neighbor_max, thr finite >= 0):      out = max_{v : dist[gt][v] <= thr} log p_v                    (eval_prob.py:389-393, var.py:504-520)
 *   mode 3 (expected_distance, param = top_k):   param == 0: out = -sum_v p_v dist[gt][v];  1 <= param <= V: the same over the top_k codes
 *          with their p renormalised to sum to 1                                                                   (var_analysis.py:252-258)
 * dist: [>= V rows][ld_dist] (modes 2 and 3; the table of varhip_code_dist_f32, ld_dist >= V), may be NULL in mode 1.  V <= 2^24.
 * Bad sizes, an unknown mode or a parameter out of its range: VARHIP_EINVAL. */
/* pinned against float64 (tests/test_token_scores_gpu.py) */
int varhip_token_score_f32(const float* logits, const int64_t* gt, int64_t ld_gt, int images, int classes, int l, int V,
                           int with_uncond, float ca, float cb, int mode, int param, float thr, const float* dist, int64_t ld_dist,
                           float* out, int64_t ld_out_img, int64_t ld_out_cls, varhip_stream_t stream);

/* ---- the distance-probability profile (VAR.distance_profile; fork var_analysis.py:352-425 plot_dist_kde: the (K, L, V) softmax, the gathered
 * (K, L, V) distances and the subsampled (d, p) pairs; :694-732 and :798-818: their mean probability per distance bin) -----------------------
 * One scale of one pass: the row layout, uncond rows, gt addressing and CFG combine of varhip_token_score_f32.  Per element v of a row whose
 * gt lies in [0, V):  p_v = vm_exp(z_v - m) / s in fp32 with m = max z and s = sum exp(z - m) of varhip_token_score_f32's row pass (the
 * exponential and the denominator of its mode 3 with param == 0; one correctly rounded division per element);  d_v = dist[gt * ld_dist + v].
 * The element is in bin b iff edges[b] <= d_v < edges[b + 1] and p_v > min_prob, every comparison in fp32: an element in no bin, a NaN d_v or
 * a NaN p_v adds nothing; a gt outside [0, V) is never dereferenced and its row adds nothing.  edges: nbins + 1 fp32 values, ascending (the
 * caller checks; the last may be +inf).  The call ADDS into
 *   count[i * ld_img + c * ld_cls + b]   the number of elements in the bin,
 *   mass_q[i * ld_img + c * ld_cls + b]  the sum over them of (int64)rint((double)p_v * 2^48)  (fixed point: a scale's cell stays <= l * 2^48),
 * with integer atomics only (LDS per workgroup, then 64-bit global adds of the non-zero bins): the sums do not depend on the order of
 * execution.  The caller zeroes both arrays once.
 * NULL operands, nbins outside [1, 256], ld_cls < nbins, ld_img < classes * ld_cls, ld_gt < l, ld_dist < V, V outside (0, 2^24], min_prob NaN,
 * negative or >= 1, images / classes / l < 1: VARHIP_EINVAL. */
/* pinned against float64 (tests/test_distance_profile_gpu.py) */
int varhip_dist_profile_f32(const float* logits, const int64_t* gt, int64_t ld_gt, int images, int classes, int l, int V,
                            int with_uncond, float ca, float cb, const float* dist, int64_t ld_dist,
                            const float* edges, int nbins, float min_prob,
                            int64_t* mass_q, int64_t* count, int64_t ld_img, int64_t ld_cls, varhip_stream_t stream);

/* ---- per-token mutual information over classes (VAR.class_information) ---------------------------------------------------------------------
 * I(c ; x_t | x_<t) = H(sum_k pi_k p_k) - sum_k pi_k H(p_k): how much the class changes the prediction at a token, without a label and without
 * the (K, L, V) softmax tensor.  One scale of one pass: the row layout, uncond rows, gt addressing and CFG combine of varhip_token_loglik_f32;
 * prior: fp32, class c of image i at prior[i * ld_prior + c] (ld_prior >= classes), used as given (not renormalised).
 * Row pass (class k of a token):  m = max z, s = sum exp(z - m) exactly as varhip_token_loglik_f32 (rowlse.h), e_v = vm_exp(z_v - m);
 *   H_k   = the `entropy` of varhip_sample_stats_f32 on that row: (float)((0 - A_k) / (double)s), A_k = sum_{e_v > 0} (double)e_v * (double)lp_v,
 *           lp_v = (z_v - m) - vm_log(s), float64 in the canonical lane order (lane i of 64: elements j * 256 + 4 * i + c ascending, lanes by the
 *           xor butterfly).  A row holding a NaN: NaN.  Written to entropy[i * ld_ent_img + k * ld_ent_cls + t].
 *   p_v   = e_v / s, one correctly rounded fp32 division.
 *   mix_q[v] += (int64)rint(((double)p_v * (double)pi_k) * 2^48)      (the product of two fp32 values is exact in float64: one rounding)
 *   hcond_q  += (int64)rint(((double)pi_k * (double)H_k) * 2^40)      (likewise; a NaN row adds nothing and raises the token's flag instead)
 *   Headroom: sum_k pi_k = 1 within 1e-6 and p_v <= 1 keep mix_q[v] <= 2^48 (1 + 1e-6) + K / 2; H_k <= ln V <= 16.7 (V <= 2^24) keeps hcond_q
 *   below 2^45.  K <= 2^31: both stay far inside int64.
 * Finalise (per token, once every class has been added):
 *   q_v = (float)((double)mix_q[v] * 2^-48);  A = sum_{q_v > 0} (double)q_v * (double)vm_log(q_v) in float64 in ONE order that depends on V
 *   alone: thread t of 256 adds its elements j * 1024 + 4 * t + c in ascending (j, c) order, the 64 lanes of a wave by the xor butterfly, the
 *   four waves as ((w0 + w1) + w2) + w3.  (The row sums use the wave order above; the token sum, which has no row pass in front of it, uses all
 *   four waves of the workgroup.)
 *   h_mix = (float)(0 - A);  h_cond = (float)(hcond_q * 2^-40);  mi = (float)((0 - A) - hcond_q * 2^-40);  logp_mix = vm_log(q_gt), NaN for a gt
 *   outside [0, V), which is never dereferenced.  A token whose flag is up (a NaN in any class row): all four are NaN.
 * Every sum across classes is an integer sum: the four per-token values are the same bits for any order of the classes (prior permuted alike),
 * any split of the classes into calls and any order of execution.
 * mix_q == NULL, the on-chip route (V <= 4096): the call holds every class of its tokens; the mixture stays in LDS, the call finalises and
 *   writes h_mix / h_cond / mi / logp_mix [i * ld_out + t] (ld_out >= l).  hcond_q, nanflag and ld_acc are not read.
 * mix_q != NULL, a chunk: the call ADDS its classes into mix_q[(i * ld_acc + t) * V + v], hcond_q[i * ld_acc + t] and raises
 *   nanflag[i * ld_acc + t] (int32, 0 / 1); ld_acc >= l; the caller zeroes the three once and runs varhip_class_mix_finish_f32 after the last
 *   chunk.  Calls that add into the same token must be ordered on one stream (a workgroup owns its token's sums).  The four outputs are not read.
 * The register path needs V % 4 == 0 and 16-byte aligned logits (V <= 4096), anything else re-reads the row from memory; V > 4096 is a chunk
 * only.  NULL operands, images / classes / l < 1, V outside (0, 2^24], ld_gt < l, ld_prior < classes, ld_ent_cls < l, ld_ent_img < classes *
 * ld_ent_cls, ld_acc < l (chunk), ld_out < l or V > 4096 (on-chip): VARHIP_EINVAL. */
/* pinned bit for bit against its host twin (tests/test_class_information_gpu.py) */
int varhip_class_mix_f32(const float* logits, const int64_t* gt, int64_t ld_gt, int images, int classes, int l, int V, int with_uncond,
                         float ca, float cb, const float* prior, int64_t ld_prior, float* entropy, int64_t ld_ent_img, int64_t ld_ent_cls,
                         int64_t* mix_q, int64_t* hcond_q, int32_t* nanflag, int64_t ld_acc, float* h_mix, float* h_cond, float* mi,
                         float* logp_mix, int64_t ld_out, varhip_stream_t stream);
/* the finalise step alone over the accumulator of chunked calls: images x l tokens, addressed as above */
int varhip_class_mix_finish_f32(const int64_t* mix_q, const int64_t* hcond_q, const int32_t* nanflag, int64_t ld_acc, const int64_t* gt,
                                int64_t ld_gt, int images, int l, int V, float* h_mix, float* h_cond, float* mi, float* logp_mix,
                                int64_t ld_out, varhip_stream_t stream);
/* the host twins: plain host code (usable without a GPU), same arguments with host pointers.  The same operations in the same order (vm_exp /
 * vm_log consist of correctly rounded operations only): the kernels' bits for 16-byte aligned logits (the twin takes the register path's order
 * iff V % 4 == 0 and V <= 4096). */
/* pinned against float64 (tests/test_class_information_cpu.py) */
int varhip_class_mix_host_f32(const float* logits, const int64_t* gt, int64_t ld_gt, int images, int classes, int l, int V, int with_uncond,
                              float ca, float cb, const float* prior, int64_t ld_prior, float* entropy, int64_t ld_ent_img, int64_t ld_ent_cls,
                              int64_t* mix_q, int64_t* hcond_q, int32_t* nanflag, int64_t ld_acc, float* h_mix, float* h_cond, float* mi,
                              float* logp_mix, int64_t ld_out);
int varhip_class_mix_finish_host_f32(const int64_t* mix_q, const int64_t* hcond_q, const int32_t* nanflag, int64_t ld_acc, const int64_t* gt,
                                     int64_t ld_gt, int images, int l, int V, float* h_mix, float* h_cond, float* mi, float* logp_mix,
                                     int64_t ld_out);

/* ---- attention mass by key scale (VAR.attention_profile) -------------------------------------------------------------------------------------
 * What the attention of reference basic_var.py:107-117 does with its probability: for every query of the current scale, how much of
 * softmax_j(q . k_j) falls on the keys of each scale and on the query's own neighbourhood, reduced where the scores are made: the (L, L) matrix
 * (depth x H x L^2 floats per image) never exists.  q: [B2][l][H*64] as varhip_gemm_qkv_f32 leaves it (normalised and scaled), kcache:
 * [B2][H][Lmax][64], keys 0 .. curL-1 valid, exactly the operands of varhip_attn_cached_f32.  The queries are the last l = pn^2 positions of the
 * cache: query t sits at key index curL - l + t, at grid position (t / pn, t % pn).  ends: a HOST array of S1 entries, ends[i] = one past the last
 * key of key scale i (strictly increasing, ends[0] >= 1, ends[S1-1] == curL, ends[S1-2] == curL - l when S1 > 1): bin i < S1 holds the keys
 * ends[i-1] <= j < ends[i]; bin S1 ("near") holds the keys j >= curL - l whose grid position is within Chebyshev distance `radius` of the
 * query's (the query itself included).
 * Arithmetic contract (what makes the kernel and the host twin bit-equal, per query):
 *   1. s_j = q . k_j: one fp32 fma chain over the 64 channels in the 4-interleaved order 0,4,1,5,2,6,3,7, 8,12,... of varhip_attn_cached_f32:
 *      the bits that kernel sees.  Keys >= curL do not exist: whatever the cache holds there has no effect (it is not read).
 *   2. m = max_j s_j (exact, order-free).
 *   3. e_j = vm_exp_le0(s_j - m) (include/var_math.h), from the same s_j.
 *   4. w_j = llrintf(e_j * 2^30): the multiply is by a power of two and exact; w_j <= 2^30, and the maximal key has w = 2^30.
 *   5. Z = sum_j w_j and W_b = sum_{j in bin b} w_j in 64-bit integers: Z >= 2^30, and curL <= 4096 keeps W <= 2^42.
 *   6. share_b = ((uint64)W_b << 21) / (uint64)Z, truncating (2^42 * 2^21 = 2^63 fits).  SHARE_ONE = 2^21; the bins b < S1 of a query sum to
 *      a value in [2^21 - S1, 2^21].
 *   7. A query with a NaN score — or with a maximum that is not finite, whose s_j - m is NaN at the maximal key — writes -1 to its S1 + 1 tokens
 *      entries, adds nothing to share_sum and adds 1 to nan_count.
 *   8. The sums over queries are integer adds (LDS, then one 64-bit global atomic per row, head, bin and workgroup): bit-equal across launch
 *      geometries and arrival orders.
 * Outputs: share_sum[b * ld_row + h * ld_head + bin] += sum over the l queries of share_bin, bins 0 .. S1; nan_count[b * H + h] += NaN queries;
 * the caller zeroes both (a second call adds again).  tokens (NULL: not written): tokens[b * ld_tok_row + h * ld_tok_head + t * (S1 + 1) + bin]
 * = share_bin of query t, plainly overwritten.  Calls that add into the same sums may run in any order.
 * VARHIP_EINVAL before any launch: a NULL q / kcache / ends / share_sum / nan_count, a size <= 0, curL > Lmax, curL > 4096, l != pn * pn,
 * l > curL, S1 outside [1, 16], ends not as above, radius < 0, q or kcache not 16-byte aligned, B2 or H above 65535. */
/* pinned bit for bit against its host twin (tests/test_attention_profile_gpu.py) */
int varhip_attn_profile_f32(const float* q, const float* kcache, int B2, int l, int H, int curL, int Lmax, const int32_t* ends, int S1,
                            int pn, int radius, int64_t* share_sum, int64_t ld_row, int64_t ld_head, int32_t* nan_count,
                            int32_t* tokens, int64_t ld_tok_row, int64_t ld_tok_head, varhip_stream_t stream);
/* the host twin: plain host code (no GPU), host pointers, the contract above query by query: the kernel's bits */
/* pinned against float64 (tests/test_attention_profile_cpu.py) */
int varhip_attn_profile_host_f32(const float* q, const float* kcache, int B2, int l, int H, int curL, int Lmax, const int32_t* ends, int S1,
                                 int pn, int radius, int64_t* share_sum, int64_t ld_row, int64_t ld_head, int32_t* nan_count,
                                 int32_t* tokens, int64_t ld_tok_row, int64_t ld_tok_head);

/* ---- where a token looks: rows of softmax(QK^T) and row vectors pushed through it (VAR.attention_maps, VAR.attention_rollout) ----------------
 * For a handful of target tokens neither the (L, L) matrix P = softmax(QK^T) of reference basic_var.py:107-117 nor a product of `depth` of
 * them is needed: a target's raw map is one row of P, its rollout (Abnar & Zuidema) a row vector pushed through the layers,
 * r <- (1 - alpha) r + alpha r Pbar_l with Pbar_l the head mean, and r P is formed tile by tile from q . k.  Two launches per layer.
 * Operands: q [B][Lq][H*64], the queries of ALL positions 0 .. Lq-1 of one block as varhip_gemm_qkv_f32 leaves them (normalised and scaled;
 * the caller stashes them scale by scale); kcache [B][H][Lmax][64], varhip_attn_cached_f32's layout, keys 0 .. Lq-1 valid.  ends: a HOST array of
 * S1 entries with the rules of varhip_attn_profile_f32 (strictly increasing, ends[0] >= 1, S1 in [1, 16]) and ends[S1-1] == Lq: query t belongs
 * to the scale i with ends[i-1] <= t < ends[i] and sees the keys j < ends[i].  No key at or beyond Lq is read.
 *
 * varhip_attn_rowstats_f32: m[(b*H + h)*Lq + t] and rinv[(b*H + h)*Lq + t], per (row, head, query):
 *   1. s_j = q_t . k_j for the visible j: one fp32 fma chain over the 64 channels in the 4-interleaved order 0,4,1,5,2,6,3,7, 8,12,... of
 *      varhip_attn_cached_f32: the bits that kernel sees.
 *   2. m = max_j s_j over the visible keys (exact, order-free; a NaN score is left out of it).
 *   3. two partial sums of vm_exp_le0(s_j - m) (include/var_math.h): A over the visible keys with (j & 4) == 0, B over those with (j & 4) != 0,
 *      each from +0 in ascending j with one rounding per add; rinv = 1.0f / (A + B), one rounding each.  The sum is >= 1 (the maximal key adds 1).
 *   4. A query with a NaN score, or with a maximum that is not finite, gets rinv = NaN (m as in 2.), and 1 is added to nan_count[b*H + h] (an
 *      integer atomic; the caller zeroes nan_count, a second call adds again).
 *
 * varhip_attn_flow_f32: r [B][T][Lq] fp32, 1 <= T <= 32; out must not overlap r.  With p_h[t][j] = vm_exp_le0(s_tj - m_t) * rinv_t (one rounding
 * for the subtraction, one for the product, s_tj as in 1.) where query t sees key j, and exactly +0 where it does not:
 *   per_head = 1: out[((b*H + h)*T + s)*Lq + j] = acc_h[s][j];  alpha is ignored
 *   per_head = 0: out[(b*T + s)*Lq + j] = fma(alpha, hsum[s][j] * (1.0f / (float)H), (1.0f - alpha) * r[b][s][j])
 * Arithmetic contract (what makes the kernel and the host twin bit-equal, per (b, s, j)):
 *   5. acc_h[s][j] is ONE fp32 fma chain acc = fma(r[b][s][t], p_h[t][j], acc) from +0 over the queries in tiles of 32, tiles ascending, inside a
 *      tile in the 4-interleaved order t = 0,4,1,5,2,6,3,7, 8,12,... (the channel order of 1.: what an MFMA 32x32x2 consumes when p comes straight
 *      out of the score registers).  The chain starts at tile floor(b0 / 32), b0 the first query of the scale that holds key 32 floor(j / 32), the
 *      first key of j's tile: the tiles before it hold no query that sees any key of j's tile and are skipped, their terms are NOT part of the
 *      chain (this matters for a non-finite r only).  From there every term is part of it, those with p = +0 and the padding of the last tile
 *      (r = p = +0) included: a term with a finite r and p = +0 leaves the bits.
 *   6. hsum[s][j] = ((+0 + acc_0) + acc_1) + ... in ascending h, one rounding per add; then one rounding each for hsum * (1/H), 1 - alpha,
 *      (1 - alpha) * r, and the final fma.  alpha = 0 returns r bit for bit where hsum is finite (and r is not -0).
 *   7. rinv_t = NaN makes p_h[t][j] NaN at every key query t sees, and 0 * NaN = NaN: such a query poisons out[b][(h)][s][j] for every s and every
 *      j it sees, in its own row b (per_head = 1: and head h) only; the keys it does not see keep their values.
 *   8. No floating-point atomics: a workgroup owns (b, 32 keys), a wave a head at a time, the heads are added by one wave in the order of 6.  The
 *      result does not depend on the launch geometry or on arrival order; a target's output does not depend on T or on the other targets.
 * A one-hot r with per_head = 1 gives rows of P: out[b][h][s][:] = p_h[t_s][:] exactly (1 * p + 0).
 * VARHIP_EINVAL before any launch, nothing written: a NULL pointer, a size <= 0, Lq > Lmax, Lq > 4096, T > 32, S1 outside [1, 16], ends not as
 * above, q or kcache not 16-byte aligned, B or H above 65535.  Both launches are timed under "other". */
/* pinned bit for bit against their host twins and within derived bars of float64 (tests/test_attn_flow_kernels_gpu.py) */
int varhip_attn_rowstats_f32(const float* q, const float* kcache, int B, int Lq, int H, int Lmax, const int32_t* ends, int S1,
                             float* m, float* rinv, int32_t* nan_count, varhip_stream_t stream);
int varhip_attn_flow_f32(const float* q, const float* kcache, const float* m, const float* rinv, const float* r, float* out, int B, int Lq, int H,
                         int Lmax, const int32_t* ends, int S1, int T, int per_head, float alpha, varhip_stream_t stream);
/* the host twins: plain host code (no GPU), host pointers, the contract above entry by entry: the kernels' bits */
/* pinned against float64 (tests/test_attn_flow_cpu.py) */
int varhip_attn_rowstats_host_f32(const float* q, const float* kcache, int B, int Lq, int H, int Lmax, const int32_t* ends, int S1,
                                  float* m, float* rinv, int32_t* nan_count);
int varhip_attn_flow_host_f32(const float* q, const float* kcache, const float* m, const float* rinv, const float* r, float* out, int B, int Lq,
                              int H, int Lmax, const int32_t* ends, int S1, int T, int per_head, float alpha);

/* ---- per-pixel class evidence (VAR.evidence_maps; fork create_heatmaps_for_classes of eval_prob.py / var_analysis.py / inpainting.py /
 * smoothing.py / var_size_analysis.py: per class and scale one bilinear F.interpolate, K full-size maps, matplotlib on the CPU) -----------
 * scores: per-token class scores, class c of image i at scores[i * ld_img + c * ld_cls + token].  The nscales selected scales are HOST arrays
 * of nscales entries each: pn (side), begin (first token; begin[s + 1] >= begin[s] + pn[s]^2) and w (weight, fp32).  ax_i: [nscales][size][2]
 * int32 (i0, i1), ax_l: [nscales][size] fp32 l1 on the device: scale s's axis table of the bilinear resample pn[s] -> size
 * (align_corners=False; the same table serves rows and columns); indices are clamped into [0, pn[s] - 1] before use.  With l0 = 1 - l1 and
 * a, b, c, d = the tokens (y.i0, x.i0), (y.i0, x.i1), (y.i1, x.i0), (y.i1, x.i1) of scale s:
 *   v_s = l0y * (l0x * a + l1x * b) + l1y * (l0x * c + l1x * d);   m = (..(0.0f + v_0 * w_0) + v_1 * w_1 ..)
 * every product, sum and difference one fp32 rounding, no contraction.
 * varhip_evidence_reduce_f32 writes, over all classes of image i:
 *   lo[i], hi[i]            min and max of m over classes and pixels
 *   pred[i][y][x]           the class with the largest m, the lowest index among exact ties
 *   margin[i][y][x]         largest minus second largest m (+inf when classes == 1)
 *   area[i][c]              pixels with pred == c (sums to size^2)
 *   maps[i][c][y][x]        m itself, only when maps != NULL
 * and nothing else; lo and hi serve as unsigned scratch during the call (integer atomic min / max on an order-preserving encoding), area is
 * zeroed by the call: no operand needs preparing.  Scores must be finite (a NaN's place in the order is not defined).
 * varhip_evidence_overlay_u8 recomputes m (it does not read maps) and writes out[i][c][y][x][3] uint8:
 *   v = (m - lo[i]) / (hi[i] - lo[i]), or m - lo[i] when hi[i] == lo[i];  bin = min((int)(v * 256), 255);  colour = matplotlib's 'jet' entry bin
 *   as uint8;  g = image[i][ch][y][x] (image_pm1: (g + 1) / 2), g8 = (uint8)clamp(g * 255, 0, 255) in fp32, truncated;
 *   out = (uint8)clamp(g8 * (1 - alpha) + colour * alpha, 0, 255) in float64 (two products, one sum), truncated.
 * image: [images][3][size][size] fp32.  out needs 4-byte alignment.
 * NULL operands (maps excepted), images / classes < 1, images > 65535 (reduce), images * classes >= 2^31 (overlay), nscales outside [1, 16],
 * pn outside [1, 64], begin negative or overlapping, more than 4096 tokens from the first selected to the last, a NaN weight, ld_cls short of
 * the last selected token, ld_img < classes * ld_cls, size outside [1, 4096], alpha outside [0, 1], image_pm1 not 0 / 1: VARHIP_EINVAL. */
/* pinned bit for bit against evidence_maps_torch (tests/test_evidence_gpu.py) */
int varhip_evidence_reduce_f32(const float* scores, int64_t ld_img, int64_t ld_cls, int images, int classes,
                               int nscales, const int* pn, const int* begin, const float* w,
                               const int* ax_i, const float* ax_l, int size,
                               float* lo, float* hi, int* pred, float* margin, int* area, float* maps, varhip_stream_t stream);
/* pinned byte for byte against evidence_maps_torch (tests/test_evidence_gpu.py) */
int varhip_evidence_overlay_u8(const float* scores, int64_t ld_img, int64_t ld_cls, int images, int classes,
                               int nscales, const int* pn, const int* begin, const float* w,
                               const int* ax_i, const float* ax_l, int size,
                               const float* lo, const float* hi, const float* image, int image_pm1, double alpha,
                               uint8_t* out, varhip_stream_t stream);
/* the 256 x 3 colour table of varhip_evidence_overlay_u8 (768 bytes); a plain host function */
/* pinned against matplotlib's 'jet' (tests/test_evidence_cpu.py) */
int varhip_evidence_jet_host(uint8_t* out);

/* ---- the pruning step of zero-shot classification (VAR.classify) ---------------------------------------------------------------------
 * One workgroup per image i.  Every candidate c < cand adds its stage's per-token scores to its float64 running total, one plain addition
 * per token in ascending token order:  totals[i * cand + c] += (double)tokens[i * ld_img + c * ld_cls + t],  t = t0 .. t1-1  (t1 == t0: the
 * totals are ranked as given and tokens may be NULL).  Then the candidates are ranked by the rule of VAR.classify: higher total first, NaN
 * below everything (-inf included), equal totals (+0 / -0, NaN / NaN) by lower index; the min(keep, cand) best indices are written to
 * kept[i * min(keep, cand) + j] in ascending index order.  keep = 1 gives the argmax of the rule.  cand <= 16384 (the totals are staged in
 * LDS); a larger cand, keep < 1, t1 < t0 or ld_cls < t1 / ld_img < cand * ld_cls with t1 > t0: VARHIP_EINVAL. */
/* pinned against a numpy lexsort of the rule (tests/test_classify_gpu.py) */
int varhip_class_select_f32(const float* tokens, int64_t ld_img, int64_t ld_cls, int images, int cand, int t0, int t1, double* totals,
                            int keep, int32_t* kept, varhip_stream_t stream);

/* ---- KV-cache row compaction (VAR.sample_best_of_pruned: the survivors of a prune boundary move to a smaller batch) ----
 * For every buffer i < nbuf:  dst[i][r][h][t][:] = src[i][idx[r]][h][t][:]  for r < rows_out, h < H, t < len, on caches laid out
 * [rows][H][Lmax][64] as SamplingEngine.workspace allocates kc[bi] / vc[bi]: src[i] has rows_src rows, dst[i] rows_dst, both H heads of Lmax
 * tokens of 64 elements of elem_bytes (4: the f32 mode, 2: f16 / bf16 caches).  Nothing else is written: tokens t >= len and rows >= rows_out of
 * dst keep their bytes.  src / dst: HOST arrays of nbuf device pointers (each 16-byte aligned), copied into the kernel's argument block like
 * varhip_edit_keep_u8's patch_nums: one launch for up to 96 buffers (the K and V caches of 48 blocks; d36 has 72), a longer list is cut into launches
 * of 96.  idx: a DEVICE array of rows_out int32 source rows, not read by the host; duplicates are allowed, and an entry outside [0, rows_src)
 * leaves its destination row unwritten.  Plain 16-byte vector loads and stores.
 * VARHIP_EINVAL before any launch: a NULL or misaligned pointer, nbuf / rows_src / rows_dst / H / Lmax <= 0, elem_bytes other than 2 or 4, len < 0
 * or > Lmax, rows_out < 0 or > rows_dst, any src range sharing a byte with any dst range (ranges = the whole buffers), a row of more than 2^31
 * 16-byte vectors.  len == 0 or rows_out == 0: success, nothing launched. */
/* pinned byte for byte against numpy's gather (tests/test_kv_compact_gpu.py) */
int varhip_kv_compact(const void* const* src, void* const* dst, int nbuf, const int32_t* idx, int rows_src, int rows_dst, int rows_out,
                      int H, int Lmax, int len, int elem_bytes, varhip_stream_t stream);

/* ---- in-place KV-cache resampling (VAR.sample_smc: dead particles' rows are overwritten by survivors') ----
 * The in-place counterpart of varhip_kv_compact on nbuf caches laid out [rows][H][Lmax][64] (elements of elem_bytes = 4 or 2).  For every row
 * r < rows with idx[r] != r:  bufs[i][r][h][t][:] = bufs[i][idx[r]][h][t][:]  for h < H, t < len.  Rows with idx[r] == r are neither read as a
 * destination nor written; nothing else is written.  The kernel checks what the host cannot (idx is a DEVICE array of rows int32, not read by
 * the host): a row whose idx[r] lies outside [0, rows), or whose source is not a fixed point (idx[idx[r]] != idx[r]), is left unwritten and
 * adds 1 to *bad once (a global atomic add; bad: a device int32 the caller zeroes).  Sources are fixed points and destinations are not, so no
 * row is both read and written: that is the whole in-place argument, and why no second cache set is needed.  bufs: a HOST array of nbuf device
 * pointers (16-byte aligned), copied into the kernel's argument block; up to 96 per launch, a longer list is cut (only the first launch counts
 * bad rows).  Plain 16-byte vector loads and stores.
 * VARHIP_EINVAL before any launch: NULL bufs / idx / bad, a NULL or misaligned buffer, nbuf / H / Lmax <= 0, rows < 0, elem_bytes other than 2
 * or 4, len < 0 or > Lmax, two buffers sharing a byte (ranges = rows whole rows), a row of more than 2^31 16-byte vectors.
 * len == 0 or rows == 0: success, nothing launched. */
/* pinned byte for byte against numpy's gather on a copy (tests/test_smc_kernels_gpu.py) */
int varhip_kv_resample(void* const* bufs, int nbuf, const int32_t* idx, int rows, int H, int Lmax, int len, int elem_bytes,
                       int32_t* bad, varhip_stream_t stream);

/* ---- the resampling decision of a particle sampler (VAR.sample_smc) ----------------------------------------------
 * One workgroup per image i < images with n particles.  tokens is addressed as in varhip_class_select_f32: tokens[i*ld_img + c*ld_cls + t].
 *   logw [images*n] float64, in and out;  seeds [images] device int64, one per image;  anc [images*n] int32 local ancestor indices in [0, n);
 *   did [images] int32, 1 if the image was resampled;  ess [images] float64, the effective sample size;  logw_seen [images*n] float64 or NULL:
 *   the log-weights after step 1, before any reset.
 * float64 with plain IEEE operations in the stated order, no contraction into FMA; varhip_smc_resample_host_f32 (host pointers, no stream)
 * gives the same bits.
 *  1. s_c = sum_{t = t0}^{t1-1} (double)tokens[..], ascending t, starting from +0.0;  logw_c = logw_c + beta * s_c.
 *  2. m = the maximum of the non-NaN logw_c.  Degenerate image (no such c, or m not finite): did = 0, ess = 0, anc = identity, logw as step 1
 *     left it.
 *  3. w_c = 0 for a NaN logw_c, otherwise (double)vm_exp((float)(logw_c - m))  (include/var_math.h).
 *  4. W = sum w_c, Q = sum w_c * w_c, both in ascending c;  ess = W * W / Q.
 *  5. The image resamples iff ess_frac < 0 (always) or ess < ess_frac * n.  Otherwise did = 0 and anc = identity.
 *  6. Systematic resampling with one uniform per (image, boundary): u = (2 (x >> 9) + 1) * 2^-24, x = word 0 of Philox4x32-10 with the image's
 *     seed as the key (split as varhip_exp1_philox_f32 splits it) and the counter (0, 0, scale, 2) (draw index 2: the fills use 0 and 1).
 *     Thresholds T_j = ((double)j + u) * (W / n), j < n;  C_c = the inclusive cumulative sum of w, ascending, C_{-1} = 0;  offspring
 *     o_c = #{j : C_{c-1} <= T_j < C_c};  a threshold not below C_{n-1} goes to the last c with w_c > 0.
 *  7. Survivors stay in place: anc[c] = c wherever o_c >= 1.  The slots with o_c = 0, in ascending order, receive the surplus copies: survivor
 *     c supplies o_c - 1 of them, survivors taken in ascending order.  Hence anc[anc[c]] == anc[c] for every c.  Every logw_c becomes +0.0,
 *     did = 1.
 * n <= 2048 (an image's weights and offspring counts are staged in 40 KiB of LDS).
 * VARHIP_EINVAL before any launch: images < 1, n < 1 or n > 2048, t0 < 0, t1 < t0, scale < 0, ld_cls < t1 or ld_img < n * ld_cls when t1 > t0,
 * a NULL operand other than logw_seen (tokens may be NULL when t1 == t0). */
/* pinned bit for bit against its host twin (tests/test_smc_kernels_gpu.py) */
int varhip_smc_resample_f32(const float* tokens, int64_t ld_img, int64_t ld_cls, int images, int n, int t0, int t1, double beta,
                            double* logw, const int64_t* seeds, int scale, double ess_frac,
                            int32_t* anc, int32_t* did, double* ess, double* logw_seen, varhip_stream_t stream);
/* pinned against a numpy restatement of the contract (tests/test_smc_resample_cpu.py) */
int varhip_smc_resample_host_f32(const float* tokens, int64_t ld_img, int64_t ld_cls, int images, int n, int t0, int t1, double beta,
                                 double* logw, const int64_t* seeds, int scale, double ess_frac,
                                 int32_t* anc, int32_t* did, double* ess, double* logw_seen);

/* ---- generative zero-shot classification (VAR.classify_generative; reference eval_prob.py:466-516) ------------------------------------------
 * Greedy CFG token selection: what var.py:172-175 + helpers.py:6-19 (fork's `gen` mode calls var.inpainting(top_k=1, top_p=0), var.py:236-364)
 * reduce to without the Exp(1) draw.  Row r = b * l + j of B * l: z = (1+t)*cond - t*uncond, rounded as cfg_sample_f32 rounds it (cond =
 * logits row r, uncond = row B*l + r), idx_out[r] = the lowest index of max(z) (+0 == -0); a row holding a NaN selects its lowest NaN index
 * (torch.argmax).  keep != NULL fuses torch.where(mask, gt_tokens, sampled) (var.py:326-328, fork): keep[b * ld_keep + j] != 0 writes
 * gt[b * ld_keep + j] and reads no logits.  Equal to cfg_sample_f32(top_k=1, top_p=0) (+ token_select_i64) on every row without an exact tie
 * at its maximum.  Bad sizes, keep without gt or ld_keep < l: VARHIP_EINVAL. */
/* pinned against varhip_cfg_sample_f32(top_k=1) (tests/test_generative_gpu.py) */
int varhip_cfg_argmax_f32(const float* logits, const uint8_t* keep, const int64_t* gt, int64_t ld_keep, int64_t* idx_out,
                          int B, int l, int V, double t_cfg, varhip_stream_t stream);

/* Feature distance of the `gen` mode (eval_prob.py:509-513, `-torch.abs(feat_input - feat_inpaint).mean(dim=-1)`): for each row r < rows,
 * score[r] = -(float)(sum_d |f_in[img[r] * D + d] - f_rec[r * D + d]| / D), the |.| in fp32 and the sum in float64 in one fixed order (thread t
 * of 256 adds d = t, t+256, ... ascending; the 256 partials by a pairwise tree), so a row's score does not depend on the rows beside it.
 * D < 1 or rows < 0: VARHIP_EINVAL. */
/* pinned against the torch L1 (tests/test_generative_gpu.py) */
int varhip_feature_l1_f32(const float* f_in, const float* f_rec, const int64_t* img, int64_t rows, int64_t D, float* score,
                          varhip_stream_t stream);

/* ---- zero-shot editing (VAR.autoregressive_infer_cfg_with_mask; demo_zero_shot_edit.ipynb cell 2: replace_embedding, the h_BChw replacement) ----
 * Keep map of every scale in one launch: keep_out[b * L + begin_s + y * pn + x] = F.interpolate(mask[b or 0][None, None], (pn, pn), 'bilinear',
 * align_corners=False)[y][x] > 0.5, and 1 on every scale with pn * pn <= 3.  mask: [Bm][h][w] fp32 (Bm == 1: one map for every row, else Bm == B),
 * patch_nums: a HOST array of S int32 (1 <= S <= 32), L = sum pn^2, keep_out: [B][L] uint8.  upsample_bilinear2d's fp32 arithmetic: scale = (float)h / pn,
 * src = max(fma(scale, d + 0.5f, -0.5f), 0), i0 = (int)src, i1 = i0 + (i0 < h - 1), l1 = src - i0, l0 = 1 - l1, then
 * v = l0h * (l0w * x00 + l1w * x01) + l1h * (l0w * x10 + l1w * x11), each operation rounded.  Bad sizes: VARHIP_EINVAL. */
/* pinned against F.interpolate > 0.5 and the reference's maps (tests/test_edit_gpu.py) */
int varhip_edit_keep_u8(const float* mask, int Bm, int h, int w, const int32_t* patch_nums, int S, int B, uint8_t* keep_out, varhip_stream_t stream);

/* varhip_quant_accum_f32 with replace_embedding fused in: position j of row b takes codebook[gt[b * ld_gt + j]] where keep[b * ld_gt + j] != 0,
 * else codebook[idx[b * pn * pn + j]].  keep / gt point at the scale's first token of a [B][ld_gt] map, ld_gt >= pn * pn.  Bitwise equal to
 * varhip_token_select_i64 into idx followed by varhip_quant_accum_f32.  Bad sizes, NULL keep or gt: VARHIP_EINVAL. */
/* pinned against varhip_token_select_i64 + varhip_quant_accum_f32 (tests/test_edit_gpu.py) */
int varhip_quant_accum_edit_f32(const int64_t* idx, const uint8_t* keep, const int64_t* gt, int64_t ld_gt, const float* codebook,
                                const int32_t* tap_idx, const float* tap_w, const float* phi_w, const float* phi_b, float ratio,
                                float* up, float* f_hat, int B, int pn, int P, int Cv, varhip_stream_t stream);

/* the more_smooth flavour: kept positions read codebook[gt[b * ld_gt + j]], the others h[b * pn * pn + j] ([B][pn*pn][Cv], the gumbel-softmax
 * embedding); bitwise equal to overwriting the kept rows of h and calling varhip_quant_accum_h_f32. */
/* pinned against an overwrite of h + varhip_quant_accum_h_f32 (tests/test_edit_gpu.py) */
int varhip_quant_accum_h_edit_f32(const float* h, const uint8_t* keep, const int64_t* gt, int64_t ld_gt, const float* codebook,
                                  const int32_t* tap_idx, const float* tap_w, const float* phi_w, const float* phi_b, float ratio,
                                  float* up, float* f_hat, int B, int pn, int P, int Cv, varhip_stream_t stream);

/* ---- nearest-codebook lookup (encode side; quant.py:150-157) --------------------------------------------
 * idx[n] = argmin_v ( |z_n|^2 + |e_v|^2 - 2 z_n.e_v ), first index on ties; z: [N][Cv], codebook: [V][Cv] */
int varhip_nearest_code_f32(const float* z, const float* codebook, int64_t* idx_out, int N, int V, int Cv, varhip_stream_t stream);

/* the same lookup for VectorQuantizer2(using_znorm=True) (quant.py:151-153): idx[n] = argmax_v (z_n / max(|z_n|,1e-12)) . (e_v / max(|e_v|,1e-12)),
 * first index on ties; every element is divided by its vector's norm before the (c-ascending fma) dot product, as F.normalize does */
int varhip_nearest_code_cos_f32(const float* z, const float* codebook, int64_t* idx_out, int N, int V, int Cv, varhip_stream_t stream);

/* ---- VectorQuantizer2.forward: the tokenizer's own pass (quant.py:52-104, vqvae.py:56-59) ------------------------------------------------
 * One scale's statistics, launched behind varhip_quant_residual_f32 of that scale (replaces quant.py:77 `idx_N.bincount(minlength=V)` and
 * quant.py:95 `F.mse_loss(f_hat, f)`).  f_hat, f: n fp32 elements each (any layout, the same for both); idx: n_idx token ids.
 *   hits[v] += |{i : idx[i] == v}| for v in [0, V) (int64, the caller zeroes the row): integer atomics only, first in LDS per workgroup
 *            (V <= 8192), then one global integer add per non-zero bin: exact and independent of the order of execution;
 *   an index outside [0, V) is neither dereferenced nor counted: *bad (int32, the caller zeroes it) += the number of such indices.  The launch
 *            is asynchronous, so the return code cannot carry it: the caller that does not trust its indices reads *bad after the stream;
 *   sum = sum_i ((double)f_hat[i] - (double)f[i])^2 in float64 in one fixed order that depends on n alone (vqstats.hip: per-thread strided
 *            partials, xor butterfly per wave, four waves in order, G = varhip_vq_stats_blocks(n) workgroup partials in scratch, added the same
 *            way by a second one-workgroup launch): no floating-point atomics, the same bits on every run;
 *   *mse_out = (float)(sum / n);  *sum_out = sum when sum_out is not NULL.
 * scratch: >= VARHIP_VQ_STATS_MAX_BLOCKS doubles.  n < 1, V < 1, n_idx < 0 or > 2^26, a NULL operand: VARHIP_EINVAL. */
#define VARHIP_VQ_STATS_MAX_BLOCKS 1024
int varhip_vq_stats_blocks(int64_t n);
/* pinned against torch.bincount and a numpy float64 sum (tests/test_vae_forward_gpu.py) */
int varhip_vq_scale_stats_f32(const float* f_hat, const float* f, int64_t n, const int64_t* idx, int64_t n_idx, int V, int64_t* hits,
                              double* scratch, double* sum_out, float* mse_out, int32_t* bad, varhip_stream_t stream);
/* quant.py:95,97: acc = 0; per scale in order acc = acc + (mse_S[si] * beta + mse_S[si]); *out = acc * (float)(1.0 / S).  fp32, every
 * operation rounded on its own (no contraction), beta as the fp32 value of the module's float. */
/* pinned against the fp32 sequence in torch (tests/test_vae_forward_gpu.py) */
int varhip_vq_loss_combine_f32(const float* mse_S, int S, float beta, float* out, varhip_stream_t stream);
/* quant.py:98 `(f_hat.data - f_no_grad).add_(f_BChw)`: v = (f_hat - f) + f per element in fp32, two roundings (not bit-equal to f_hat).
 * f_hat, f: [B][HW][C] channels-last; out_nhwc (nullable) the same layout, out_nchw (nullable) [B][C][HW], both written in the one pass;
 * at least one of them.  Bad sizes: VARHIP_EINVAL. */
/* pinned against (f_hat - f) + f in torch, bit for bit (tests/test_vae_forward_gpu.py) */
int varhip_vq_straight_through_f32(const float* f_hat, const float* f, float* out_nhwc, float* out_nchw, int B, int HW, int C,
                                   varhip_stream_t stream);

/* ---- validation metrics (VAR.evaluate; reference trainer.py:54-84 eval_ep, :126-156 the L_* / acc_* / z_voc_usage logging block) -------------
 * One scale of one pass, launched behind the head of that scale; replaces trainer.py:72-75 (F.cross_entropy and argmax over the (B, L, V)
 * logits tensor) and :140,151-153 without that tensor.  logits: the head's fp32 output, R rows of l tokens, row r * l + t; gt[r * ld_gt + t]
 * the ground-truth token; the four outputs share one addressing, out[r * ld_out + t].  With z the row:
 *   nll    = -((z_gt - max z) - log(sum exp(z - max z))): the negated value of varhip_token_loglik_f32 for the same row, bit for bit (one piece
 *            of device code, rowlse.h);
 *   pred   = the lowest index of max z (+0 == -0); a row holding a NaN gives its lowest NaN index (torch.argmax; varhip_cfg_argmax_f32's rule);
 *   rank   = |{v : z_v > z_gt or (z_v == z_gt and v < gt)}| (varhip_token_score_f32's total order; a NaN compares false);
 *   smooth = (float)((double)z_gt - sum / V), sum = sum_v (double)z_v in float64 in one order that depends on V alone (lane i of 64 adds the
 *            elements j * 256 + 4 * i + c in ascending (j, c) order, the lanes by the xor butterfly 32 .. 1);
 *            nn.CrossEntropyLoss(label_smoothing=e) of the row is nll + e * smooth.
 * A token outside [0, V) is never dereferenced: nll = smooth = NaN, rank = -1 (pred is still the row's argmax).  V < 2^24.
 * On a row holding a NaN, nll is what varhip_token_loglik_f32 gives there (NaN when z_gt is the NaN; otherwise its register path drops the NaN
 * element from the exponential sum and its scalar path propagates it) and smooth is NaN.
 * Bad sizes (R, l, V < 1, ld_gt < l, ld_out < l) or a NULL operand: VARHIP_EINVAL. */
/* pinned against float64, torch.argmax and the rank's definition (tests/test_evaluate_gpu.py) */
int varhip_token_eval_f32(const float* logits, const int64_t* gt, int64_t ld_gt, int R, int l, int V, float* nll, float* smooth,
                          int64_t* pred, int32_t* rank, int64_t ld_out, varhip_stream_t stream);
/* Once per call, over the [N][ld] per-token arrays varhip_token_eval_f32 filled; begin_S1: a HOST array of S + 1 int32 token offsets, begin[0] = 0,
 * strictly ascending, begin[S] = L <= ld, 1 <= S <= 32.  Per scale s (replaces the per-scale loop of trainer.py:149-155 and the sums of :72-75):
 *   nll_S[s], smooth_S[s] = the float64 sums over the N * l_s tokens of the scale, every addition in float64 in one fixed order that depends on
 *            (N, l_s) alone: element i = image * l_s + token, thread t of 256 adds i = t, t + 256, ... ascending, a wave its lanes by the xor
 *            butterfly, the workgroup its four waves in order (the scheme of varhip_vq_scale_stats_f32); no floating-point atomics;
 *   correct_S[s] = |{tokens with rank == 0}| (int64; an out-of-range gt has rank -1 and never counts).
 * pred_hist_V[v] += |{tokens with pred == v}| (int64, the caller zeroes it; replaces trainer.py:140 bincount): integer atomics only, in LDS
 * first for V <= 8192; a pred outside [0, V) is not counted.  N * L <= 2^26.  Bad sizes or a NULL operand: VARHIP_EINVAL. */
/* pinned against numpy float64 sums and torch.bincount (tests/test_evaluate_gpu.py) */
int varhip_eval_reduce_f32(const float* nll, const float* smooth, const int64_t* pred, const int32_t* rank, int64_t ld, int N,
                           const int32_t* begin_S1, int S, int V, double* nll_S, double* smooth_S, int64_t* correct_S,
                           int64_t* pred_hist_V, varhip_stream_t stream);

/* ---- the logit lens (VAR.logit_lens): a block's prediction against the final one ----------------------------------------------------------
 * One scale of one pass.  logits: the head applied to the residual stream behind a block, final_logits: the head's output behind the last
 * block, both [R * l][V] fp32 with row r, token t at r * l + t; gt[r * ld_gt + t] the ground-truth token; the five outputs share one
 * addressing, out[r * ld_out + t].  With z the layer's row, zf the final row, m = max z, mf = max zf (exact, order-free):
 *   nll, pred, rank: varhip_token_eval_f32's on the layer row, bit for bit (one piece of device code, rowlse.h, on the same path: both rows in
 *            registers where V % 4 == 0, V <= 4096 and BOTH operands are 16-byte aligned; two passes over memory otherwise).  A token outside
 *            [0, V) is never dereferenced: nll = NaN, rank = -1.  Ties and NaN rows as there.
 *   With d_v = z_v - m, df_v = zf_v - mf (fp32, one rounding each), e_v = vm_exp(d_v), ef_v = vm_exp(df_v) (include/var_math.h),
 *            S = sum_v e_v,  A = sum_{e_v > 0} e_v * d_v,  Sf = sum_v ef_v,  B = sum_{ef_v > 0} ef_v * (df_v - d_v)
 *        every product, difference and addition of the four sums in float64, in ONE order that depends on V alone (varhip_token_eval_f32's
 *        `smooth` order: lane i of 64 adds the elements j * 256 + 4 * i + c in ascending (j, c) order, the lanes by the xor butterfly 32 .. 1),
 *        and ls = vm_log((float)S), lsf = vm_log((float)Sf):
 *   entropy = (float)((double)ls - A / S)                     -sum_v p_v log p_v of the layer row in nats, in [0, log V]
 *   kl      = (float)((B / Sf - (double)lsf) + (double)ls)    KL(pf || p) = sum_v pf_v (log pf_v - log p_v)
 *        Neither depends on which path ran (they do not use the row pass's fp32 sum).  ef_v == 0 adds nothing whatever z_v is; ef_v > 0
 *        against z_v = -inf gives +inf; a NaN difference (a NaN element, a +inf maximum, a row of -inf) in the layer row makes entropy and kl
 *        NaN, in the final row kl.  Equal rows, one pointer or equal contents: B = +0, lsf == ls, kl = +0.0 exactly.
 * V < 2^24.  VARHIP_EINVAL before any launch, nothing written: a NULL operand, R, l, V < 1, ld_gt < l, ld_out < l. */
/* pinned bit for bit against its host twin and against varhip_token_eval_f32 (tests/test_logit_lens_kernels_gpu.py) */
int varhip_token_lens_f32(const float* logits, const float* final_logits, const int64_t* gt, int64_t ld_gt, int R, int l, int V,
                          float* nll, float* entropy, float* kl, int64_t* pred, int32_t* rank, int64_t ld_out, varhip_stream_t stream);
/* the host twin: plain host code (no GPU), host pointers, the contract above row by row: the kernel's bits on 16-byte aligned device operands
 * (host addresses carry no alignment constraint: the register path's row pass is taken wherever V % 4 == 0 and V <= 4096) */
/* pinned against float64 (tests/test_logit_lens_cpu.py) */
int varhip_token_lens_host_f32(const float* logits, const float* final_logits, const int64_t* gt, int64_t ld_gt, int R, int l, int V,
                               float* nll, float* entropy, float* kl, int64_t* pred, int32_t* rank, int64_t ld_out);

/* ---- activation patching (VAR.patch_effects): ablate or replace column ranges of an activation matrix, in place ---------------------------------
 * act: [rows * l][ld] fp32, row r, token t at (r * l + t) * ld; only columns below `width` are ever touched (ld > width: the padding stays).
 * It is the attention output in front of proj (width C, head h at columns 64 h .. 64 h + 63) or the MLP hidden activation behind the GELU
 * (width hidden).  dir: a DEVICE array (the host twin: a host array) of n_dir directives of four int32 (row, c0, c1, src); a directive
 * rewrites act[row][t][c0 .. c1 - 1] for every token t of the row:
 *   src == -1   +0.0f
 *   src == -2   the column's mean over the row's l tokens, m_c = s / (float)l: s is the fp32 sum of act[row][t][c] in ascending t, one
 *               rounding per add, starting from the t = 0 element; the division is one correctly rounded fp32 division.  l == 1: the bits stay.
 *   src >= 0    act[src][t][c], token by token; no directive of the same launch may write those columns of row src (the caller's duty).
 * A directive is skipped whole, and writes nothing, where row is outside [0, rows), src is outside [-2, rows), c0 < 0, c1 > width, c0 >= c1,
 * or c0 or c1 is no multiple of 4.  Directives of one launch that name the same row have disjoint column ranges (the caller's duty).
 * n_dir == 0: success without a launch (dir may be NULL).  VARHIP_EINVAL before any launch, nothing written: n_dir < 0, a NULL operand with
 * n_dir > 0, rows, l or width < 1, ld < width, ld % 4 != 0, act not 16-byte aligned, width above 2^22.
 * A bandwidth kernel: 16-byte loads and stores, the lanes of a wave on consecutive column groups, no LDS; the one lane that owns a column
 * group of a mean directive walks t, so the sum has one order. */
/* pinned bit for bit against its host twin (tests/test_patch_kernels_gpu.py) */
int varhip_act_patch_f32(float* act, int64_t ld, int rows, int l, int width, const int32_t* dir, int n_dir, varhip_stream_t stream);
/* the host twin: plain host code (no GPU), host pointers, the directives one after the other: the kernel's bits (a NaN's payload aside) */
/* pinned against the numpy restatement tests/patchref.py (tests/test_patch_cpu.py) */
int varhip_act_patch_host_f32(float* act, int64_t ld, int rows, int l, int width, const int32_t* dir, int n_dir);
/* varhip_adaln_block_f32 with interventions: the same seven launches, varhip_act_patch_f32(att, C, B2, l, C, dir_att, n_att) between attention
 * and proj, varhip_act_patch_f32(hid, hidden, B2, l, hidden, dir_hid, n_hid) between fc1 and fc2.  An empty table launches nothing:
 * n_att == n_hid == 0 issues exactly the seven launches and leaves varhip_adaln_block_f32's bits.  VARHIP_EINVAL before any launch: what
 * varhip_adaln_block_f32 refuses, a negative count, a non-empty table that is NULL or whose matrix is NULL or not 16-byte aligned,
 * n_hid > 0 with hidden % 4 != 0.  f32 only. */
/* pinned bit for bit against varhip_adaln_block_f32 (tests/test_patch_kernels_gpu.py) and against weight surgery (tests/test_patch_effects_gpu.py) */
int varhip_adaln_block_patched_f32(float* x, float* x2, float* xn, float* q, float* att, float* hid,
                                   const float* ada, int64_t ld_ada,
                                   const float* qkv_w, const float* qkv_b, const float* scale_mul, float plain_scale, int l2norm,
                                   const float* proj_w, const float* proj_b, const float* fc1_w, const float* fc1_b,
                                   const float* fc2_w, const float* fc2_b, float* kcache, float* vcache,
                                   int B2, int l, int C, int H, int hidden, int pos0, int Lmax, float eps,
                                   const int32_t* dir_att, int n_att, const int32_t* dir_hid, int n_hid, varhip_stream_t stream);
/* varhip_adaln_block_f32 with varhip_attn_keysel_f32(q, kcache, vcache, att, B2, l, H, pos0 + l, Lmax, ends, S1, keymask) in the place of
 * varhip_attn_cached_f32: the same seven launches, and with full masks varhip_adaln_block_f32's bits.  The new keys and values are appended
 * to the caches whatever the masks say (a mask hides keys from this block's queries only).  VARHIP_EINVAL before any launch: what either
 * refuses.  f32 only. */
/* pinned bit for bit against varhip_adaln_block_f32 (tests/test_knockout_kernels_gpu.py) */
int varhip_adaln_block_keysel_f32(float* x, float* x2, float* xn, float* q, float* att, float* hid,
                                  const float* ada, int64_t ld_ada,
                                  const float* qkv_w, const float* qkv_b, const float* scale_mul, float plain_scale, int l2norm,
                                  const float* proj_w, const float* proj_b, const float* fc1_w, const float* fc1_b,
                                  const float* fc2_w, const float* fc2_b, float* kcache, float* vcache,
                                  int B2, int l, int C, int H, int hidden, int pos0, int Lmax, float eps,
                                  const int32_t* ends, int S1, const int32_t* keymask, varhip_stream_t stream);

/* ---- direct logit attribution (VAR.logit_attribution): the final logit of a token as a sum over what was written into the residual stream ----
 * The head is W (LN(x) (1 + s) + sh) + b with an affine-free LayerNorm (var.py:118-124), the stream a plain sum (basic_var.py:157-158).  With
 * r = W[a] - W[b'] (no rival: r = W[a]), g = r (1 + s), mu and sigma the LayerNorm statistics of the final x (biased variance, eps inside the
 * root) and ghat = (g - mean(g)) / sigma:   r . (LN(x) (1 + s) + sh) + b_a - b_b' = ghat . x + konst,  konst = r . sh + b_a - b_b'.
 *
 * The target of every token of one scale of one pass.  logits: [R * l][V] fp32, row r, token t at r * l + t; gt[r * ld_gt + t] the target
 * token a, against[r * ld_gt + t] (mode 2 only; NULL otherwise) the rival; rival and value share one addressing, out[r * ld_out + t].
 *   mode 0   no rival:  rival = -1, value = z_a
 *   mode 1   rival = the exact arg-max of z over v != a, the lowest index on ties;  value = z_a - z_rival (one fp32 subtraction)
 *   mode 2   rival = against;  value = z_a - z_rival
 * One pass over the row.  Nothing here depends on an order of summation (a maximum, an index, one subtraction), so the row is read with 16-byte
 * loads where V % 4 == 0 and logits is 16-byte aligned and with scalar loads otherwise, to the same bits; rowlse.h's row pass (max and exp-sum)
 * has nothing to add.  A token (or, in mode 2, a rival) outside [0, V) is never dereferenced: rival = -1, value = NaN.  A row that holds a NaN
 * anywhere: rival = -1, value = NaN, in every mode.  V == 1 in mode 1 (no rival exists): rival = -1, value = NaN.
 * V < 2^24.  VARHIP_EINVAL before any launch, nothing written: a NULL operand (against: in mode 2), a mode outside 0 .. 2, R, l, V < 1,
 * ld_gt < l, ld_out < l. */
/* pinned bit for bit against its host twin (tests/test_dla_kernels_gpu.py) */
int varhip_dla_target_f32(const float* logits, const int64_t* gt, const int64_t* against, int64_t ld_gt, int mode, int R, int l, int V,
                          int64_t* rival, float* value, int64_t ld_out, varhip_stream_t stream);
/* the host twin: plain host code (no GPU), host pointers, the contract above row by row */
/* pinned against the numpy restatement tests/dlaref.py (tests/test_dla_cpu.py) */
int varhip_dla_target_host_f32(const float* logits, const int64_t* gt, const int64_t* against, int64_t ld_gt, int mode, int R, int l, int V,
                               int64_t* rival, float* value, int64_t ld_out);
/* The direction of every token of one scale of one pass.  x: the final residual stream [R * l][C] fp32 (dense); hn_scale[r * ld_hn + c] and
 * hn_shift[r * ld_hn + c] the head's modulation s and sh of row r; head_w [V][C] and head_b [V] the head; tok_a[r * ld_tok + t] the target
 * token, tok_b[r * ld_tok + t] the rival (tok_b == NULL: no rival for any token).  Outputs: ghat [R * l][C] fp32 (dense), konst and gx (double)
 * at out[r * ld_out + t].  Per token, every operation below in float64 on the widened fp32 inputs (a product of two fp32 values is exact):
 *   r_c = W[a][c] - W[b'][c]  (no rival: W[a][c]),   g_c = r_c * (1.0 + s_c)
 *   S1 = sum_c x_c,  S2 = sum_c x_c * x_c,  G = sum_c g_c,  K = sum_c r_c * sh_c
 *   mu = S1 / C,  var = max(S2 / C - mu * mu, 0),  sigma = sqrt(var + (double)eps),  mg = G / C          (correctly rounded division and root)
 *   ghat_c = (float)((g_c - mg) / sigma)                                                  rounded to fp32 once
 *   gx = sum_c (double)ghat_c * x_c  (with the rounded ghat),   konst = K + (b_a - b_b')   (no rival: K + b_a)
 * The five sums have ONE order that depends on C alone, varhip_token_lens_f32's: lane i of 64 adds its elements j * 256 + 4 * i + c in
 * ascending (j, c) order from +0.0, the 64 lanes by the xor butterfly 32 .. 1.  One wave per token, 16-byte loads and stores, no atomics.
 * A target or a rival outside [0, V) is never dereferenced: that token's ghat, konst and gx are NaN.
 * VARHIP_EINVAL before any launch, nothing written: a NULL operand (tok_b aside), R, l, C, V < 1, C % 4 != 0, ld_hn < C or ld_hn % 4 != 0,
 * ld_tok < l, ld_out < l, a negative or NaN eps, x, hn_scale, hn_shift, head_w or ghat not 16-byte aligned, konst or gx not 8-byte aligned. */
/* pinned bit for bit against its host twin (tests/test_dla_kernels_gpu.py) */
int varhip_dla_direction_f32(const float* x, const float* hn_scale, const float* hn_shift, int64_t ld_hn, const float* head_w,
                             const float* head_b, const int64_t* tok_a, const int64_t* tok_b, int64_t ld_tok, int R, int l, int C, int V,
                             float eps, float* ghat, double* konst, double* gx, int64_t ld_out, varhip_stream_t stream);
/* the host twin: plain host code (no GPU), host pointers, the operations above in the stated order: the kernel's bits (a NaN's payload aside) */
/* pinned against the numpy restatement tests/dlaref.py (tests/test_dla_cpu.py) */
int varhip_dla_direction_host_f32(const float* x, const float* hn_scale, const float* hn_shift, int64_t ld_hn, const float* head_w,
                                  const float* head_b, const int64_t* tok_a, const int64_t* tok_b, int64_t ld_tok, int R, int l, int C,
                                  int V, float eps, float* ghat, double* konst, double* gx, int64_t ld_out);
/* Segmented row dots in float64: out[m * nseg + s] = sum over the columns j of segment s (width C / nseg) of (double)a[m * lda + j] *
 * (double)b[m * ldb + j], m < M.  ldb == 0 reads one vector b for every row (a bias).  nseg == 1: ghat against a kept stream; nseg == H: u
 * against the attention output, head by head.  The products are exact; the sum has ONE order that depends on (C, nseg) alone: with q = C /
 * nseg / 4 the segment's groups of four columns and P the largest power of two <= min(64, q), lane i of P adds the groups i, i + P, ... in
 * ascending order, the four columns of a group in order, from +0.0; the P lanes by the xor butterfly P / 2 .. 1.  A wave works on 64 / P
 * consecutive (row, segment) pairs.  A bandwidth kernel: 16-byte loads, consecutive lanes on consecutive groups, 8 flops per 32 bytes; it is
 * bounded by the 4 M C (ldb == 0) or 8 M C bytes it reads.
 * VARHIP_EINVAL before any launch, nothing written: a NULL operand, M, C or nseg < 1, C % nseg != 0, a segment width that is no multiple
 * of 4, lda < C, ldb neither 0 nor >= C, lda or ldb no multiple of 4, a or b not 16-byte aligned, out not 8-byte aligned. */
/* pinned bit for bit against its host twin (tests/test_dla_kernels_gpu.py) */
int varhip_rowdot_seg_f64(const float* a, int64_t lda, const float* b, int64_t ldb, int M, int C, int nseg, double* out, varhip_stream_t stream);
/* the host twin: plain host code (no GPU), host pointers, the stated order */
/* pinned against the numpy restatement tests/dlaref.py (tests/test_dla_cpu.py) */
int varhip_rowdot_seg_host_f64(const float* a, int64_t lda, const float* b, int64_t ldb, int M, int C, int nseg, double* out);

/* ==== 16-bit-input throughput mode ("f16") ===================================================================
 * The reference's harness runs the path under torch.autocast('cuda', dtype=torch.float16) (demo_sample.py:66-68): every F.linear of
 * basic_var.py then computes in fp16 and attention takes the flash path with fp16 q/k/v (basic_var.py:97,113).  These entry points are
 * that mode on MI355X: fp16 operands (`void*` = _Float16 data), fp32 accumulation on v_mfma_f32_*_f16, fp32 bias / GELU / AdaLN gate /
 * residual, one rounding where an output is fp16.  They are NOT under the fp32 bit-exactness contract (the MFMA-internal reduction over
 * k is not a k-ascending chain): tests compare them with the CPU twin (oracle/var_oracle.py, f16=True: the fp32 restatement with the same
 * rounding points) within a stated tolerance.  LayerNorm, GroupNorm, softmax statistics, the sampler and the quantizer stay fp32. */

/* out[m][n] = epi(sum_k A[m][k] W[n][k] + bias[n]); A: [M][lda] fp16, W: [N][ldw] fp16, bias / gamma fp32, out and resid fp16 or fp32
 * (out_f16 / resid_f16).  epi as varhip_gemm_nt_f32.  Requires K % 64 == 0, N % 4 == 0, lda/ldw % 8 == 0, 16-byte aligned pointers.
 * replaces F.linear at basic_var.py:93,119,52 and var.py:124 under fp16 autocast. */
int varhip_gemm_nt_f16(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias,
                       void* out, int64_t ldo, int out_f16, int M, int N, int K, int epi,
                       const void* resid, int64_t ldr, int resid_f16, const float* gamma, int64_t ldg, int rows_per_group,
                       int batch, int64_t sA, int64_t sW, int64_t sO, varhip_stream_t stream);
/* testing / experiments: force the tile of the following f16 GEMM calls (0: 128x128, 1: 64x64, 2: 256x256 with 8 waves; -1: automatic choice) */
int varhip_gemm16_force_tile(int tile);
/* experiments / tests: 1 (default) = whole 256x256 tiles run on the persistent kernel k_gemm16p (one workgroup per CU walking a tile list),
 * 0 = on k_gemm16<8,4,2,4> (one workgroup per tile).  Identical results. */
int varhip_gemm16_persistent(int on);
/* tests: 1 (default, or what VARHIP_GEMM16_DEEP seeded at load) = the 64-row kernels with three / four LDS stages, 0 = k_gemm16<2,2> (gemm_nt) and
 * k_gemm16<2,4> (gemm_qkv) with two.  Identical results. */
int varhip_gemm16_deep(int on);
/* testing: the kernel that launch i (0 or 1: a GEMM may go out as two launches over row ranges) of the latest varhip_gemm_nt_* / varhip_gemm_qkv_*
 * call of either flavour ran, written by the launcher from its own template arguments just before the launch (forcing a tile is a request, this is
 * what ran), as the decimal number  TMW * 1000 + TNW * 100 + WN * 10 + NST  of k_gemm16<TMW, TNW, 2, WN, NST>:
 *   4422 128x128; 1124 32x32, four stages; 2224 64x64, four stages; 2222 64x64, two stages; 6442 192x256; 8442 256x256;
 *   1423 / 2423 / 2422 the q/k/v kernels of 32 / 64 / 64 rows x 128 columns with three / three / two stages; 8440 = k_gemm16p, the persistent 256x256 kernel.
 * 0: the call made no such launch (and before the first call); a refused call (VARHIP_EINVAL) leaves both unchanged.  Host only. */
int varhip_gemm16_last_pick(int i);
/* mat_qkv + q/k L2-norm + scale + KV-cache append (basic_var.py:93-109): fp16 x fp16 -> fp32 -> fp16 q [M][C] and fp16 caches [B2][H][Lmax][64] */
int varhip_gemm_qkv_f16(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, int M, int C, int K,
                        const float* scale_mul, float plain_scale, int l2norm,
                        void* q_out, void* kcache, void* vcache, int B2, int l, int H, int pos0, int Lmax, varhip_stream_t stream);
/* attention over the fp16 KV cache (basic_var.py:107-117 on the flash path): fp32 scores and softmax, p rounded to fp16 for p.v, fp16 out */
int varhip_attn_cached_f16(const void* q, const void* kcache, const void* vcache, void* out,
                           int B2, int l, int H, int curL, int Lmax, varhip_stream_t stream);
/* testing: the waves per workgroup (NW of k_attn16<NW>, 1 .. 4; a wave owns 32 queries, the grid is ceil(l / (32 NW)) x H x B2) of the latest
 * varhip_attn_cached_f16 / _bf16 launch, written by the launcher from the value it switches on.  0 before the first launch; a refused call
 * (VARHIP_EINVAL) leaves it unchanged.  Read-only: it changes no dispatch.  Host only: it launches nothing and reads no device memory. */
int varhip_attn16_last_waves(void);
/* varhip_ln_modulate_f32 with the result rounded to fp16 (the A operand of the next GEMM) */
int varhip_ln_modulate_f16out(const float* x, const float* scale, int64_t ld_scale, const float* shift, int64_t ld_shift,
                              void* out, int M, int C, int rows_per_group, float eps, varhip_stream_t stream);
/* one AdaLNSelfAttn block (basic_var.py:152-159) in this mode: fp32 residual stream and AdaLN parameters, fp16 GEMM operands and KV cache */
int varhip_adaln_block_f16(float* x, float* x2, void* xn16, void* q16, void* att16, void* hid16, const float* ada, int64_t ld_ada,
                           const void* qkv_w16, const float* qkv_b, const float* scale_mul, float plain_scale, int l2norm,
                           const void* proj_w16, const float* proj_b, const void* fc1_w16, const float* fc1_b,
                           const void* fc2_w16, const float* fc2_b, void* kcache16, void* vcache16,
                           int B2, int l, int C, int H, int hidden, int pos0, int Lmax, float eps, varhip_stream_t stream);

/* the decoder's convolutions in this mode (basic_vae.py:22-28,40-60,163-226 under fp16 autocast): fp16 channels-last activations and
 * weights ([Cout][3][3][Cin], or the phase form of varhip_upconv_pack_f32 rounded to fp16), fp32 bias, fp16 residual and output;
 * out_mode 1 / 2: the last conv writes fp32 NCHW, de-normalised to [0,1] / clamped to [-1,1].  gn_part (nullable): per-block
 * per-channel (sum, sum of squares) of the ROUNDED result, as varhip_conv3x3_gn_nhwc_f32.  Cin % 32 == 0. */
int varhip_conv3x3_nhwc_f16(const void* in, const void* w, const float* bias, const void* resid, void* out, double* gn_part,
                            int B, int H, int W, int Cin, int Cout, int out_mode, varhip_stream_t stream);
int varhip_upconv_phase_f16(const void* in, const void* w_phase, const float* bias, void* out, double* gn_part,
                            int B, int H, int W, int Cin, int Cout, varhip_stream_t stream);
/* ResnetBlock's `conv(swish(norm(x)))` (basic_vae.py:57-60) in ONE launch: `in` is the RAW 16-bit map, table [B][2][Cin] fp32 its GroupNorm as one
 * multiply-add per element (varhip_gn_scale_shift_f32 below: scale = rstd * gamma, shift = beta - mean * scale), silu != 0: swish.  The normalisation
 * runs on the convolution's input patch in LDS, so the apply pass over the map (varhip_gn_apply_f16: one read + one write of every activation)
 * disappears.  Bit-identical to varhip_gn_apply_f16 followed by varhip_conv3x3_nhwc_f16 (out_mode 0; bias, resid, gn_part as there).  Shapes:
 * varhip_conv16_gn_fusable(B, H, W, Cin, Cout) != 0 (maps that tile into 8 x 32 or 16 x 16 patches with a workgroup for every CU, Cout % 128 == 0 or
 * % 160 == 0, the table within the LDS budget: Cin <= 320 at 8 x 32 patches); VARHIP_EINVAL otherwise — the caller then runs the two launches. */
int varhip_conv16_gn_fusable(int B, int H, int W, int Cin, int Cout);
int varhip_gnconv3x3_nhwc_f16(const void* in, const float* table, int silu,
                              const void* w, const float* bias, const void* resid, void* out, double* gn_part,
                              int B, int H, int W, int Cin, int Cout, varhip_stream_t stream);
/* table[b][0][c] = stats[b][g(c)].rstd * gamma[c], table[b][1][c] = beta[c] - stats[b][g(c)].mean * table[b][0][c]   (what varhip_gn_apply_* forms per channel) */
int varhip_gn_scale_shift_f32(const float* stats, const float* gamma, const float* beta, float* table, int B, int C, int G, varhip_stream_t stream);
/* testing / experiments: force the pixel tile of the following f16 convolutions (2: 128 pixels, 4 waves, two workgroups per CU;
 * 4: 256 pixels, 8 waves, two workgroups per CU; 8: the halo-patch kernel where the shape allows it; anything else: by size) */
int varhip_conv16_force_tile(int wm);
/* testing: the kernel instantiation that the latest varhip_conv3x3_nhwc_*, varhip_gnconv3x3_nhwc_* or varhip_upconv_phase_* call of either flavour
 * launched (forcing is a request, this is what ran), as the decimal number  nz * 1000 + GN * 100 + TNW * 10 + kernel:
 *   kernel  0 = k_conv16 on 128-pixel tiles, 3 = k_conv16 on 256-pixel tiles, 1 / 2 = k_conv16h on 8 x 32 / 16 x 16 halo patches
 *   TNW     channels per tile / 32: 5, 4 (either kernel), 2, 1 (128-pixel tiles only: a forced 4 on them reports kernel 0)
 *   GN      1 = the GroupNorm-fused form of k_conv16h (varhip_gnconv3x3_nhwc_*)
 *   nz      1 = a 3x3 convolution, 4 = the four phases of varhip_upconv_phase_*
 * e.g. 1051 = k_conv16h<5, 32, false>, 1142 = k_conv16h<4, 16, true>, 4043 = k_conv16<4, 3, 4, 2> in the phase form, 1010 = k_conv16<1, 4, 2>.
 * -1 before the first launch; a refused call (VARHIP_EINVAL) leaves it unchanged.  Host only: it launches nothing and reads no device memory. */
int varhip_conv16_last_pick(void);
/* GroupNorm on fp16 [B][HW][C] (basic_vae.py:18-19): statistics in fp64, affine + optional SiLU in fp32, fp16 result */
int varhip_gn_stats_f16(const void* x, float* stats, double* scratch, int B, int HW, int C, int G, float eps, varhip_stream_t stream);
int varhip_gn_apply_f16(const void* x, const float* stats, const float* gamma, const float* beta, void* out,
                        int B, int HW, int C, int G, int silu, varhip_stream_t stream);
/* casts at the edges of the mode (n % 4 == 0, 16-byte aligned) */
/* the decoder's tail in one pass (basic_vae.py:224-226 norm_out -> swish -> conv_out, the caller's clamp vqvae.py:63 and (x + 1) / 2 var.py:190):
 * out = clamp(conv3x3(SiLU(GroupNorm(x))) + bias) as fp32 NCHW (out_mode 2) or de-normalised to [0, 1] (out_mode 1); stats [B][G][2] = (mean, rstd).
 * Bit-identical to varhip_gn_apply_f16 followed by varhip_conv3x3_nhwc_f16.  Shapes it does not take (H % 8, W % 32, Cin % 32, Cout > 16): VARHIP_EINVAL. */
int varhip_gn_silu_conv_out_f16(const void* x, const float* stats, const float* gamma, const float* beta, const void* w, const float* bias,
                                float* out, int B, int H, int W, int Cin, int Cout, int G, int out_mode, varhip_stream_t stream);
int varhip_cast_f32_to_f16(const float* in, void* out, int64_t n, varhip_stream_t stream);
int varhip_cast_f16_to_f32(const void* in, float* out, int64_t n, varhip_stream_t stream);

/* ---- the same mode with bfloat16 storage ("bf16"; the reference's other 16-bit option: utils/arg_util.py `fp16: int  # 1: using fp16, 2: bf16`,
 * trainer / AmpOptimizer autocast dtype, utils/amp_sc.py).  One entry point per _f16 entry point above, same arguments and meaning with
 * `void*` = bfloat16 data (the out_f16 / resid_f16 flags then mean bfloat16): the same kernels compiled with the bf16 MFMA opcodes and conversions
 * (var_amd/csrc/elem16.h).  Rounding points as in the fp16 flavour; 8 significant bits instead of 11, fp32's exponent range. */
int varhip_gemm_nt_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias,
                       void* out, int64_t ldo, int out_f16, int M, int N, int K, int epi,
                       const void* resid, int64_t ldr, int resid_f16, const float* gamma, int64_t ldg, int rows_per_group,
                       int batch, int64_t sA, int64_t sW, int64_t sO, varhip_stream_t stream);
int varhip_gemm16_force_tile(int tile);
int varhip_gemm16_persistent(int on);
int varhip_gemm16_deep(int on);
int varhip_gemm16_last_pick(int i);
int varhip_gemm_qkv_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, int M, int C, int K,
                        const float* scale_mul, float plain_scale, int l2norm,
                        void* q_out, void* kcache, void* vcache, int B2, int l, int H, int pos0, int Lmax, varhip_stream_t stream);
int varhip_attn_cached_bf16(const void* q, const void* kcache, const void* vcache, void* out,
                           int B2, int l, int H, int curL, int Lmax, varhip_stream_t stream);
int varhip_ln_modulate_bf16out(const float* x, const float* scale, int64_t ld_scale, const float* shift, int64_t ld_shift,
                              void* out, int M, int C, int rows_per_group, float eps, varhip_stream_t stream);
int varhip_adaln_block_bf16(float* x, float* x2, void* xn16, void* q16, void* att16, void* hid16, const float* ada, int64_t ld_ada,
                           const void* qkv_w16, const float* qkv_b, const float* scale_mul, float plain_scale, int l2norm,
                           const void* proj_w16, const float* proj_b, const void* fc1_w16, const float* fc1_b,
                           const void* fc2_w16, const float* fc2_b, void* kcache16, void* vcache16,
                           int B2, int l, int C, int H, int hidden, int pos0, int Lmax, float eps, varhip_stream_t stream);
int varhip_conv3x3_nhwc_bf16(const void* in, const void* w, const float* bias, const void* resid, void* out, double* gn_part,
                            int B, int H, int W, int Cin, int Cout, int out_mode, varhip_stream_t stream);
int varhip_upconv_phase_bf16(const void* in, const void* w_phase, const float* bias, void* out, double* gn_part,
                            int B, int H, int W, int Cin, int Cout, varhip_stream_t stream);
int varhip_gnconv3x3_nhwc_bf16(const void* in, const float* table, int silu,
                               const void* w, const float* bias, const void* resid, void* out, double* gn_part,
                               int B, int H, int W, int Cin, int Cout, varhip_stream_t stream);
int varhip_conv16_force_tile(int wm);
int varhip_gn_stats_bf16(const void* x, float* stats, double* scratch, int B, int HW, int C, int G, float eps, varhip_stream_t stream);
int varhip_gn_apply_bf16(const void* x, const float* stats, const float* gamma, const float* beta, void* out,
                        int B, int HW, int C, int G, int silu, varhip_stream_t stream);
int varhip_gn_silu_conv_out_bf16(const void* x, const float* stats, const float* gamma, const float* beta, const void* w, const float* bias,
                                 float* out, int B, int H, int W, int Cin, int Cout, int G, int out_mode, varhip_stream_t stream);
int varhip_cast_f32_to_bf16(const float* in, void* out, int64_t n, varhip_stream_t stream);
int varhip_cast_bf16_to_f32(const void* in, float* out, int64_t n, varhip_stream_t stream);


/* ---- per-kernel timing (bench.py's roofline leg) -----------------------------------------------------------
 * When enabled, every launch is bracketed by hipEvents on its own stream and its algorithmic FLOPs and bytes are
 * accumulated per kernel family.  varhip_timing_read synchronises the recorded events.
 * families: 0 gemm (the 128x128-tile instantiation k_dma_gemm<4,4,false,2,false>), 1 conv3x3 (the 128x160-tile implicit-GEMM
 * instantiation k_dma_gemm<4,5,true,2,false>), 2 attn, 3 sampler, 4 ln, 5 qkv_prep, 6 gn, 7 other, 8 gemm_small (every other tile
 * of the transformer GEMMs and the element-wise-load fallback), 9 conv_small (every other conv tile: nearest-2x gather, Cout not
 * a multiple of 160); the 16-bit mode's kernels in families of their own (one arithmetic type, hence one MFMA peak, per family):
 * 10 gemm16 (k_gemm16p, the persistent 256x256-tile kernel), 11 gemm16_small (every k_gemm16 tile), 12 conv16h (k_conv16h<5,32>),
 * 13 conv16_small (every other fp16 conv kernel), 14 attn16; 15 conv_wino (k_conv3x3_wino, the fused Winograd F(2x2,3x3) conv; its FLOPs
 * are the executed multiplies, 16 per 2x2 tile, so it is not priced as a direct conv).  Families 0, 1, 10 and 12 each map to exactly
 * one kernel symbol and 15 to the instantiations of one template (k_conv3x3_wino<residual, partials, 0>), so their averages can be checked
 * against a rocprofv3 kernel trace.  16 attn_profile (k_attn_profile, varhip_attn_profile_f32: FLOPs = both QK^T passes).
 * 17 conv_wino_up (k_conv3x3_wino_up, the Upsample2x convs as position-sparse Winograd; FLOPs = the executed multiplies, 9 per 2x2 tile;
 * a family of its own so that conv_wino keeps counting the ResnetBlock convs alone).  Returns the number of families. */
#define VARHIP_NFAM 18
int varhip_timing_enable(int on);
/* restrict the timing to the families whose bit is set (default: all).  Every timed launch costs two event records on the stream —
 * about 2 % of a sampling call when all ~3000 launches are timed; bench.py times only what its roofline object reports. */
int varhip_timing_select(int family_mask);
int varhip_timing_reset(void);
int varhip_timing_read(double* ms, double* flops, double* bytes, int64_t* launches);
const char* varhip_timing_name(int family);

#ifdef __cplusplus
}
#endif
#endif /* VAR_HIP_H */
