/*
 * osrl_amd.h -- C ABI of libosrl_amd.so: the MI355X (gfx950) kernels behind the
 * OSRL Trainer.train_one_step() hot path (BC / CPQ / BCQ-Lag / CDT).
 *
 * The reference (liuzuxin/OSRL) is pure Python on PyTorch aten and has NO FFI seam
 * (SURVEY.md section 8b); the seam this library fills is "what aten did for the
 * reference": each entry point below names the reference code it replaces.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to fp32 (row-major) unless stated otherwise;
 *    nn.Linear weights are [out,in] exactly as in the reference state_dict;
 *  - caller allocates every output and workspace; nothing is allocated or freed here;
 *  - every call is asynchronous on `stream` (a hipStream_t passed as void*), makes no
 *    host synchronisation and is hipGraph-capturable;
 *  - return value: 0 on success, otherwise a hipError_t (or -1 for a bad argument);
 *    nothing throws across the ABI.  State: none that persists between calls, with ONE opt-in exception --
 *    osrl_args_begin / osrl_args_end bracket a THREAD-LOCAL argument arena (csrc/argmem.h, a static thread_local in
 *    csrc/optim.hip): between the two calls the fused-MLP / optimizer / prologue launches of the calling thread record
 *    or look up their descriptors there; outside such a bracket (the default) every call is stateless and re-entrant
 *    across streams, devices and threads.  A few entry points own caller-provided device scratch that must be zero
 *    before the first call and is re-armed by the call itself (arrival counters: osrl_mlp_backward_dw_tiles_adam,
 *    osrl_mlp_backward_dz_seed, osrl_mlp_regress_step, the *_ws loss / quantile calls).
 */
#ifndef OSRL_AMD_H
#define OSRL_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OSRL_MAX_LAYERS 4 /* Linear layers per MLP */
#define OSRL_MAX_NETS 8   /* ensemble members sharing one input tile */
#define OSRL_MAX_WIDTH 1024 /* widest layer (input, hidden or output) of an MLP */
/* MLP widths: nets whose dims are all <= 448 run on the fused 16-row-tile kernels (a whole net per tile in LDS, four
 * waves of at most 7 column blocks of 16).  A net with any dims[l] in 449..1024 takes the WIDE PATH of osrl_mlp_*:
 * one launch per layer (grid = row tile x column group x net, ensembles in one launch), fp32 MFMA on the same packed
 * Wf / Wb copies, bias + activation + out_scale (forward) or act'(h) (backward) in the launch's epilogue, layer 0 read
 * from the virtual input (osrl_rows_t: maps, src1) directly.  Its contract differs from the fused one in three
 * points:
 *   - every intermediate output is the next launch's input: forward needs h[e][l] for every l < n_layers - 1 and
 *     backward needs dz[e][l] for every layer above the lowest one asked for (dz or dx); else OSRL_E_UNSUPPORTED;
 *   - tails run as their own launches behind the layers (the named glue calls), forward2 is two launches, row_list
 *     returns -3, the wg_cap / tile_rows / share0 hints are ignored;
 *   - osrl_mlp_backward_dz_seed honours the seed (dY by the tile kernel on the output layer alone, outputs <= 448
 *     wide; wider: OSRL_E_UNSUPPORTED); osrl_mlp_regress_step returns OSRL_E_UNSUPPORTED. */

enum { OSRL_ACT_ID = 0, OSRL_ACT_RELU = 1, OSRL_ACT_TANH = 2 };
/* row r of the virtual input maps to source row: r | r % div | r / div
 * (MOD = torch.tile(obs[None],(N,1,1)) cpq.py:170-174 ; DIV = repeat_interleave bcql.py:138) */
enum { OSRL_MAP_ID = 0, OSRL_MAP_MOD = 1, OSRL_MAP_DIV = 2 };

/* A stack of n_layers Linear(+activation) layers for n_nets ensemble members:
 * osrl/common/net.py:12-30 `mlp()`; ensembles net.py:208-287. */
typedef struct {
  int32_t n_layers, n_nets;
  int32_t dims[OSRL_MAX_LAYERS + 1]; /* in, h1, ..., out */
  int32_t acts[OSRL_MAX_LAYERS];     /* activation after each layer */
  float out_scale;                   /* net output = out_scale * act(z)  (act_limit of net.py:62,85,339) */
  int32_t tile_rows;                 /* tuning hint: rows per workgroup tile (0 = auto, else 16 / 32 / 64);
                                      * 80 = forward-only launches take the one-workgroup-per-CU kernel when the
                                      * network's shape allows it */
  int32_t wg_cap;                    /* forward launches: at most this many workgroups in the grid (0 = one per
                                      * tile); a capped launch walks its tiles, leaving CU slots to concurrent
                                      * latency-critical launches */
  /* PACKED weights (osrl_pack_weights): Wf feeds forward, Wb (packed W^T) feeds backward-dz.
   * Wf[e][l]: PF[k/4][n][k%4], n < round16(out), k < round16(in), zero padded.
   * Wb[e][l]: PB[o/4][i][o%4], i < round16(in)+16, o < round16(out), zero padded (NULL if unused). */
  const float* Wf[OSRL_MAX_NETS][OSRL_MAX_LAYERS];
  const float* Wb[OSRL_MAX_NETS][OSRL_MAX_LAYERS];
  const float* b[OSRL_MAX_NETS][OSRL_MAX_LAYERS]; /* [dims[l+1]] canonical bias */
} osrl_mlp_t;

/* One canonical nn.Linear weight [out,in] (row-major, at src_flat + src_off) and where its packed
 * copies go (float offsets into pf / pb; negative = skip). */
typedef struct {
  int64_t src_off, f_off, b_off;
  int32_t out, in;
} osrl_pack_entry_t;

/* Virtual input matrix [rows, d0+d1] = cat(src0[map0(r)], src1[map1(r)]) -- replaces the
 * torch.cat / tile / repeat_interleave copies of net.py:232,273,320,337 and cpq.py:170. */
typedef struct {
  int32_t rows;
  int32_t d0, map0, div0;
  int32_t d1, map1, div1;
  const float* src0;
  const float* src1; /* may be NULL when d1 == 0 */
  /* Optional (both NULL = none): a launch over a row SET chosen on the device -- row r of the virtual input is row
   * row_list[r] of the matrix described above, and only the first min(rows, *n_rows_dev) rows exist (rows = the list's
   * capacity: it sizes the grid; workgroups past the count leave at once).  For cpq.py:183-184: of the N*B sampled actions
   * only those whose KL reaches the batch quantile enter qc_ood -- the target cost critics run on those rows alone.
   * Honoured by the 80-row inference forward of <= 256-wide nets (osrl_mlp_forward); every other entry point returns -3. */
  const int32_t* row_list;
  const int32_t* n_rows_dev;
  /* Optional (0 = off): SHARED SRC0 ROWS of an inference launch whose rows are n * div0 + b (map0 = OSRL_MAP_MOD: cpq.py:164-176,
   * N sampled actions per observation).  share0 = 1: tiles are [copies] x [16 src0 rows] and the part of layer 0 that lies in
   * the first 16 * share_k16 input columns (all of them columns of src0; share_k16 >= 1, at least one 16-column k-step left)
   * is computed once per src0 row of a tile instead of once per launch row.  Same products, another order of a row's sum (a few
   * ulp from the plain launch): for no_grad launches.  Needs div0 % 16 == 0 and (rows / div0) a multiple of the tile's row
   * blocks (5; 4 on the 64-row form).  A HINT: taken by the 80-row inference forward of <= 256-wide (4-wave) and 400-wide
   * (8-wave) nets (osrl_mlp_forward[_tail]); every other launch computes the same function on its plain tiles. */
  int32_t share0, share_k16;
} osrl_rows_t;

/* Activations written by forward / read by backward.  h[e][l] = post-activation output of
 * layer l of net e, [rows, dims[l+1]].  h[e][n_layers-1] (the net output) is REQUIRED in
 * forward; every other pointer may be NULL (= not saved). */
typedef struct {
  float* x; /* [rows, dims[0]] the concatenated input (needed by dW of layer 0) */
  float* h[OSRL_MAX_NETS][OSRL_MAX_LAYERS];
} osrl_mlp_acts_t;

typedef struct {
  const float* dy[OSRL_MAX_NETS]; /* [rows, dims[L]] grad wrt the net's (post-activation) output */
  float* dz[OSRL_MAX_NETS][OSRL_MAX_LAYERS]; /* out (NULL = skip): grad wrt pre-activation of layer l */
  float* dx[OSRL_MAX_NETS]; /* out (NULL = skip): [rows, dx_cols] = dX[:, dx_col0 : dx_col0+dx_cols] */
  int32_t dx_col0, dx_cols;
} osrl_mlp_grads_t;

/* Optional row-local tail of a fused-MLP launch, applied by the workgroup that owns the rows while its last tile is
 * still in LDS (one launch and one global round trip less on the step's latency chain).  HOST struct.
 *   OSRL_TAIL_VAE_LATENT      forward of the VAE encoder (net 0, output [rows, 2L] = mean | log_std):
 *                             out[rows, L] = mean + exp(clamp(log_std, -4, 15)) * eps        == osrl_vae_latent
 *   OSRL_TAIL_VAE_LATENT_BWD  backward of the VAE decoder whose dX slice (dx[0], dx_cols == L) is dL/dz:
 *                             out[rows, 2L] = d(recon + beta KL)/d(mean | log_std)          == osrl_vae_latent_bwd
 *                             with head = the encoder output [rows, 2L]; beta, rows_global as in that call
 *   OSRL_TAIL_GAUSS           forward of a squashed-Gaussian actor trunk (net 0, output [rows, 2L] = mu | log_std, L =
 *                             action_dim; net.py:152-205): up to two action draws and the N pre-tanh OOD draws of
 *                             cpq.py:164-176 from the LDS-resident head tile --
 *                               out [rows, L]  = max_action * tanh(mu + exp(clamp(log_std, -20, 2)) * eps)    == osrl_gauss_head
 *                               out2 [rows, L] = the same with eps2 (NULL = none), tanh2 [rows, L] = its tanh(u) (optional)
 *                               out_ood [n_samples * rows, L], row j * rows + r = mu + sd * eps_ood[j, r, :]  == osrl_gauss_ood_sample
 *                             (any of the three may be absent: eps / eps2 / eps_ood NULL) */
/*   OSRL_TAIL_VAE_KL          forward of the VAE encoder (net 0, output [rows, 2L]): out[rows] = mean_k KL(N(mean_k, sd_k) || N(0, 1)),
 *                             the per-row statistic of cpq.py:178-182                                      == osrl_vae_kl_rows
 *                             (fused into the 80-row N*B-row kernel's output pass; a launch of its own behind any other) */
enum { OSRL_TAIL_NONE = 0, OSRL_TAIL_VAE_LATENT = 1, OSRL_TAIL_VAE_LATENT_BWD = 2, OSRL_TAIL_GAUSS = 3, OSRL_TAIL_VAE_KL = 4 };
typedef struct {
  int32_t kind;
  int32_t L;
  const float* eps;  /* [rows, L] */
  const float* head; /* OSRL_TAIL_VAE_LATENT_BWD only */
  float* out;
  float beta;          /* OSRL_TAIL_VAE_LATENT_BWD only */
  int32_t rows_global; /* OSRL_TAIL_VAE_LATENT_BWD only: the loss is a mean over this many rows (<= 0: rows) */
  float inv_rows_;     /* filled in by the library */
  /* OSRL_TAIL_GAUSS only */
  float max_action;
  const float* eps2;
  float* out2;
  float* tanh2;
  const float* eps_ood;
  float* out_ood;
  int32_t n_samples, pad_;
} osrl_mlp_tail_t;

/* One weight-gradient GEMM  dW[out,in] = dz^T a,  db[out] = sum_rows dz  (autograd of addmm). */
typedef struct {
  const float* dz; /* [rows, out] */
  const float* a;  /* [rows, in]  */
  int64_t w_off, b_off; /* float offsets of dW / db inside one gradient slab */
  int32_t out, in;
  int32_t ldz, lda;     /* row strides of dz / a in floats (0 = dense: out / in) */
} osrl_dw_entry_t;

/* Device-resident per-step scalars, advanced once per train step by osrl_step_tick(). */
typedef struct {
  int64_t step;     /* optimizer step count t (1-based after the first tick) */
  float bc1;        /* 1 - beta1^t */
  float bc2_sqrt;   /* sqrt(1 - beta2^t) */
  float lr_scale;   /* LambdaLR factor min(t/warmup,1) (cdt.py:327-330); 1 when warmup == 0 */
  uint32_t arrive_; /* workgroup arrival counter of osrl_step_begin (0 between launches) */
} osrl_step_state_t;

/* One dropout site (HOST struct, read at launch): probability, site id (unique per nn.Dropout call site and
 * layer), generator seed, and the device step state whose `step` decorrelates successive train steps. */
typedef struct {
  float p;
  uint32_t site;
  uint64_t seed;
  const osrl_step_state_t* st;
} osrl_dropout_t;

/* ---- fused MLP (mlp.hip): replaces nn.Sequential(Linear,act,...) forward + its autograd ---- */
/* lds_bytes / tile selection are internal; rows may be any value >= 1. */
int osrl_mlp_forward(const osrl_mlp_t* net, const osrl_rows_t* in, const osrl_mlp_acts_t* out, void* stream);
/* Two independent forward problems in one launch (e.g. the actor on next_obs and on obs, cpq.py:141,164): same
 * results as two osrl_mlp_forward calls; falls back to exactly that when the two tile shapes differ. */
int osrl_mlp_forward2(const osrl_mlp_t* net0, const osrl_rows_t* in0, const osrl_mlp_acts_t* out0,
                      const osrl_mlp_t* net1, const osrl_rows_t* in1, const osrl_mlp_acts_t* out1, void* stream);
int osrl_mlp_backward_dz(const osrl_mlp_t* net, int32_t rows, const osrl_mlp_acts_t* saved,
                         const osrl_mlp_grads_t* g, void* stream);
/* The same launches followed by a row-local tail (osrl_mlp_tail_t; NULL or kind NONE = the plain call): results are
 * those of the plain call plus the named glue call (net.py:319-331 reparameterisation and its autograd, cpq.py:125-131),
 * fused into the launch when its last tile is LDS-resident, two launches otherwise. */
int osrl_mlp_forward_tail(const osrl_mlp_t* net, const osrl_rows_t* in, const osrl_mlp_acts_t* out,
                          const osrl_mlp_tail_t* tail, void* stream);
/* osrl_mlp_forward2 with a forward tail per problem (either may be NULL): e.g. the actor on next_obs and on obs with
 * every action draw of the CPQ step (cpq.py:141,159,164-176,209) made by the same launch. */
int osrl_mlp_forward2_tail(const osrl_mlp_t* net0, const osrl_rows_t* in0, const osrl_mlp_acts_t* out0,
                           const osrl_mlp_tail_t* tail0, const osrl_mlp_t* net1, const osrl_rows_t* in1,
                           const osrl_mlp_acts_t* out1, const osrl_mlp_tail_t* tail1, void* stream);
int osrl_mlp_backward_dz_tail(const osrl_mlp_t* net, int32_t rows, const osrl_mlp_acts_t* saved,
                              const osrl_mlp_grads_t* g, const osrl_mlp_tail_t* tail, void* stream);
/* The backward launch COMPUTES the gradient it starts from (new; the reference's autograd starts from a loss scalar,
 * cpq.py:133,151,198,220): the loss kernels between a forward and a backward launch (osrl_vae_loss,
 * osrl_cpq_critic_loss, osrl_cpq_cost_loss, osrl_cpq_actor_loss, osrl_gauss_head_bwd) only turn forward outputs of the
 * SAME ROWS into dL/d(output) plus one logged batch sum -- here every row tile evaluates that expression for its rows
 * while it stages dY (g->dy is ignored and may be NULL), and the statistic is the fixed-order sum of per-tile partials
 * taken by the last workgroup to finish (wait-free: partials are device-coherent words, one arrival atomic per
 * workgroup at its very end).  dL/d(output) has the bits of the named loss kernel; the statistic is the same sum in a
 * different (fixed) order.  Kinds, with y_e = output of net e of this launch and inv = 1 / rows_global (<= 0: rows):
 *   OSRL_SEED_MSE        dy = 2 (y - x0[r, c]) scale;   stat = sum (y - x0)^2 * stat_scale
 *                        [+ kl_beta * stat_scale2 * sum_{r, k < kl_L} KL(kl_head[r, k], kl_head[r, kl_L + k]) if kl_head]
 *                        (VAE: x0 = actions, scale = stat_scale = inv / ad, stat_scale2 = inv / L; == osrl_vae_loss)
 *   OSRL_SEED_CPQ_CRITIC backup = x0[r] + gamma (1 - x1[r]) 1[min_e b_e[r] <= thres] min_e a_e[r];  dy_e = 2 (y_e - backup) inv
 *                        (a = target critics [n_a, rows], b = target cost critics, x0 = rewards, x1 = done; == osrl_cpq_critic_loss)
 *   OSRL_SEED_CPQ_COST   backup = x0[r] + gamma min_e a_e[r];  dy_e = 2 (y_e - backup) inv       (== osrl_cpq_cost_loss, MSE part)
 *   OSRL_SEED_CPQ_ACTOR  dy_e = -1[min b_e[r] <= thres] inv if e == argmin_e a_e[r] else 0; stat = -sum mask min_e a_e * inv
 *                        (a = the critics' outputs [n_a, rows] = this launch's nets, b = the cost critics'; == osrl_cpq_actor_loss)
 *   OSRL_SEED_GAUSS_HEAD dy[r, :] = d/d(mu | log_std) of a = max_action tanh(mu + sd eps) given dL/da = sum_e a_e[r, :]
 *                        (a = [n_a, rows, ad] input gradients, tanh_u / eps [rows, ad]; no statistic; == osrl_gauss_head_bwd)
 *   OSRL_SEED_BCQ_CRITIC backup = x0[r] + gamma (1 - x1[r]) max_j [ thres min(q1_j, q2_j) + (1 - thres) max(q1_j, q2_j) ] over the
 *                        n_samples target samples j of row r (a = [n_a + n_b, rows * n_samples] target outputs, row-major by
 *                        sample: r * n_samples + j; q1 = min over the first n_a, q2 over the last n_b; thres = lambda of
 *                        bcql.py:144-146; x1 may be NULL: no (1 - done)); dy_e = 2 (y_e - backup) inv      (== osrl_bcq_critic_loss)
 *   OSRL_SEED_FQE        fitted Q evaluation of a frozen policy: the launch's nets are n_a reward critics followed by n_b cost
 *                        critics (n_a + n_b = n_nets, each <= 4), a = their targets' outputs [n_a + n_b, rows] on (s', pi(s'));
 *                        net e bootstraps from target e alone (no minimum over members: they stay independent estimates):
 *                          backup_e = (e < n_a ? x0[r] : b[r]) + gamma (1 - x1[r]) a[e rows + r];  dy_e = 2 (y_e - backup_e) scale
 *                        (x0 = rewards, b = costs, x1 = done, scale = stat_scale = inv).  TWO statistics: the squared errors
 *                        of the reward nets are the tile's first partial, those of the cost nets its second;
 *                          stat[0] = stat_scale sum_{e < n_a, r} (y_e - backup_e)^2,  stat2[0] = stat_scale sum_{e >= n_a, r} (.)^2
 *                        (either may be NULL) = the sum over members of the batch-mean squared error (net.py:240-242)
 *   OSRL_SEED_GAUSS_NLL  the diagonal-Gaussian dynamics member (algorithms/dynamics.py, probabilistic=True): every net's output
 *                        row is (od + 1 means | raw cost | od + 1 raw log-variances), NL = 2 od + 3, x0 = the target table
 *                        [rows, od + 2], lo = gamma and hi = thres are the log-variance bounds (lo < hi).  For c < od + 1:
 *                          lv1 = hi - softplus(hi - raw_c), lv_c = lo + softplus(lv1 - lo), raw_c = y[od + 2 + c],
 *                          softplus(x) = max(x, 0) + log1p(exp(-|x|));
 *                          dy[c]          = 2 (y_c - x0_c) exp(-lv_c) scale
 *                          dy[od + 1]     = 2 (y - x0) scale                                  (the cost column: MSE)
 *                          dy[od + 2 + c] = (1 - (y_c - x0_c)^2 exp(-lv_c)) sigmoid(hi - raw_c) sigmoid(lv1 - lo) scale
 *                          stat = stat_scale sum_{nets, r} [ sum_{c < od + 1} ((y_c - x0_c)^2 exp(-lv_c) + lv_c) + (y_{od+1} - x0_{od+1})^2 ]
 * partials: >= 2 * n_nets * ceil(rows / 16) floats of scratch; counter: one uint32, ZERO before the first launch
 * (re-armed by the launch).  HOST struct. */
enum { OSRL_SEED_NONE = 0, OSRL_SEED_MSE = 1, OSRL_SEED_CPQ_CRITIC = 2, OSRL_SEED_CPQ_COST = 3, OSRL_SEED_CPQ_ACTOR = 4,
       OSRL_SEED_GAUSS_HEAD = 5, OSRL_SEED_BCQ_CRITIC = 6, OSRL_SEED_FQE = 7, OSRL_SEED_GAUSS_NLL = 8 };
typedef struct {
  int32_t kind;
  int32_t n_a, n_b;
  int32_t rows_global;
  const float *a, *b;
  const float *x0, *x1;
  const float *eps, *tanh_u;
  const float* kl_head;
  int32_t kl_L, n_samples;
  float gamma, thres, scale, max_action;
  float stat_scale, stat_scale2, kl_beta, pad2_;
  float* partials;
  uint32_t* counter;
  float* stat;
  float* stat2; /* OSRL_SEED_FQE only: the second statistic (every other kind ignores it) */
} osrl_mlp_seed_t;
int osrl_mlp_backward_dz_seed(const osrl_mlp_t* net, int32_t rows, const osrl_mlp_acts_t* saved,
                              const osrl_mlp_grads_t* g, const osrl_mlp_tail_t* tail, const osrl_mlp_seed_t* seed,
                              void* stream);
/* ---- one supervised regression step of one MLP in ONE launch (mlp.hip mlp_step_kernel) -------------------------
 * BCTrainer.train_one_step (osrl/algorithms/bc.py:45-55,103-109 with the minibatch of examples/train/train_bc.py:105-121):
 *   [sample + gather the minibatch] -> forward -> F.mse_loss -> backward -> dW / db -> Adam (+ refresh of the packed
 *   weight copies) -> step tick (+ the previous step's statistics into the ring)
 * i.e. exactly osrl_step_begin + osrl_mlp_forward + osrl_mse_loss + osrl_mlp_backward_dz + osrl_mlp_backward_dw_tiles +
 * osrl_adam_step_packed on the same arguments, with the same parameter bits (same MFMA chains, same summation orders,
 * same element-wise update); the loss statistic is summed per 16-row tile and then in tile order (deterministic, not
 * the single-workgroup order of osrl_mse_loss).  At B = 256 those six launches are ~53 us of mostly launch gaps; here
 * the row tiles (16 rows, 8 waves) run gather / forward / loss / backward back to back out of LDS, signal an
 * arrival counter, and the dW tile workgroups -- which cover ALL rows, so there are no gradient slabs -- apply Adam to
 * their tile from LDS.  One grid-wide dependency instead of five launch boundaries.
 * Requirements (else OSRL_E_UNSUPPORTED and nothing is launched; callers keep the six-launch plan): one net; widest
 * layer 129..448 (the 8-wave 16-row tile of the fused MLP kernels); rows <= 16 * OSRL_STEP_MAX_WG; a dW work list in
 * osrl_mlp_backward_dw_tiles' format with ONE row split per tile and <= OSRL_STEP_MAX_WG items; weight decay 0; no
 * target copy.  ws: OSRL_STEP_WS floats of device scratch, zero before the first call, owned by this step (the kernel
 * re-arms its counters; ws[OSRL_STEP_MAX_WG + 2] != 0 afterwards = a workgroup gave up waiting, results invalid).
 * All workgroups of the launch must be resident at once (<= OSRL_STEP_MAX_WG of 256 CUs: they are). HOST struct. */
#define OSRL_STEP_MAX_WG 128
#define OSRL_STEP_WS (OSRL_STEP_MAX_WG + 8)
#define OSRL_E_UNSUPPORTED (-2)
typedef struct {
  /* osrl_step_begin's state arguments */
  osrl_step_state_t* st;
  float beta1, beta2;
  int32_t warmup, n_stats, ring_len;
  /* osrl_replay_gather's arguments; n_fields = 0: the minibatch is already in `in` / `target` */
  int32_t n_fields;
  const float* stats_cur;
  float* ring;
  const float* src[8];
  float* dst[8];
  int32_t width[8];
  float scale[8];
  int64_t n_rows;
  uint64_t gather_seed;
  uint32_t gather_stream, pad0_;
  /* osrl_replay_gather_n's live row count (device int64; n_rows is then the tables' capacity); NULL (zero) = n_rows */
  const int64_t* n_rows_dev;
  /* osrl_mlp_forward / osrl_mlp_backward_dz's arguments (grads.dy[0] = the loss gradient buffer, written here) */
  osrl_mlp_t net;
  osrl_rows_t in;
  osrl_mlp_acts_t acts;
  osrl_mlp_grads_t grads;
  /* osrl_mse_loss's arguments */
  const float* target; /* [rows, dims[L]] */
  int64_t n_global;    /* elements the mean runs over (<= 0: rows * dims[L]) */
  float* stat;         /* optional */
  /* osrl_mlp_backward_dw_tiles's arguments; tile_blocks = 4 (64 x 64 tiles) or 2 (32 x 32: four times the
   * workgroups on a quarter of the MFMA work each -- what a 256-row batch wants; same bits, the sum order of an
   * output element depends on its rows-per-wave only) */
  const osrl_dw_entry_t* entries;
  const int32_t* work;
  int32_t n_work, tile_blocks;
  /* osrl_adam_step_packed's arguments (n_splits = 1, no target, weight decay 0) */
  float *p, *m, *v;
  const int32_t *map_f, *map_b;
  float *pf, *pb;
  float lr, eps;
  float* ws;
  /* osrl_replay_gather_w's table (device uint64[n_rows], osrl_weights_cum_u64); NULL (zero) = uniform draws */
  const uint64_t* cum;
} osrl_mlp_step_t;
int osrl_mlp_regress_step(const osrl_mlp_step_t* s, void* stream);

/* ---- the VAE's forward and backward on the training rows as ALL-CU layer launches (vae_ns.hip, round 5) -------------
 * VAE.forward + the reconstruction / KL loss + its autograd through decoder and encoder (osrl/common/net.py:290-339,
 * osrl/algorithms/cpq.py:125-135 == bcql.py:122-133 == bearl.py vae_loss): the same results in the same buffers as
 *   osrl_mlp_forward_tail(enc, VAE_LATENT) -> osrl_mlp_forward(dec) -> osrl_mlp_backward_dz_seed(dec, MSE + KL statistic,
 *   VAE_LATENT_BWD tail) -> osrl_mlp_backward_dz(enc)
 * (statistic and gradients equal up to fp32 summation order), launched differently: at 2048 rows a fused 16-row-tile
 * launch of a 400-wide net occupies 128 of the 256 CUs and spends most of its time walking the 400 x 400 layer; here
 * every H x H layer is one launch of [48 rows x 80 columns] output tiles over ALL CUs (4 waves split K, operands
 * requested k-steps ahead, partial tiles meet in LDS), the narrow first layers are one launch for both nets, and the
 * narrow heads / the latent's dX ride as split-K partial rows ("slabs", one per 80-column group) in the epilogue of the
 * wide launch that produces their input and are summed by the prologue of the launch that consumes them:
 *   forward : l0 (enc layer 0 | the observation part of dec layer 0) -> enc wide (+ head slabs) -> dec wide (prologue:
 *             head = sum slabs, z = mean + sd eps, h0 = relu(P + Wz z + b); + output slabs)
 *   backward: dec wide^T (prologue: u = max_action tanh(sum slabs), dY of the MSE, dZ2, the logged loss; A operand =
 *             (dZ2 W2) * relu'(h1); epilogue: dZ0 = . * relu'(h0), + dL/dz slabs) -> enc wide^T (prologue: dL/d(mean |
 *             log_std) through z and the KL term)
 * Requirements (osrl_vae_ns_supported; else callers keep the fused launches): both nets [in, H, H, out] with relu, relu,
 * (id | tanh); H % 80 == 0, 80 <= H <= 448; obs + act <= 128 and obs + L <= 128 columns; L <= 16; act <= 16.
 * HOST struct; every pointer is device memory.  enc / dec: n_nets 1, n_layers 3 (the descriptors of the fused launches). */
typedef struct {
  const osrl_mlp_t* enc;     /* [od + ad, H, H, 2 L]  relu, relu, id   (mean | log_std) */
  const osrl_mlp_t* dec;     /* [od + L,  H, H, ad]   relu, relu, tanh, out_scale = max_action */
  int32_t rows, od, ad, L;
  int32_t rows_global;       /* the loss is a mean over this many rows (<= 0: rows) */
  float beta;                /* KL weight (cpq.py:129) */
  const float *obs, *act, *eps; /* [rows, od], [rows, ad], [rows, L] */
  osrl_mlp_acts_t enc_acts;  /* out: x [rows, od + ad], h[0][0..1] [rows, H], h[0][2] = head [rows, 2 L] */
  osrl_mlp_acts_t dec_acts;  /* out: x [rows, od + L],  h[0][0..1] [rows, H], h[0][2] = u [rows, ad] */
  float* z;                  /* out [rows, L] */
  osrl_mlp_grads_t enc_g;    /* out: dz[0][0..2] (backward) */
  osrl_mlp_grads_t dec_g;    /* out: dz[0][0..2] (backward) */
  float* P;                  /* scratch [rows, H] */
  float* slabs;              /* scratch 3 * (H / 80) * rows * 32 floats */
  float* partials;           /* scratch 2 * ceil(rows / 48) floats: per-tile partials of the logged loss */
  uint32_t* counter;         /* one word, ZERO before the first launch (re-armed by the launch) */
  float* stat;               /* out: loss_vae = mse + beta * kl (cpq.py:127-129) */
} osrl_vae_ns_t;
int osrl_vae_ns_supported(const osrl_vae_ns_t* v);   /* 1 / 0; no launch */
int osrl_vae_ns_forward(const osrl_vae_ns_t* v, void* stream);
int osrl_vae_ns_backward(const osrl_vae_ns_t* v, void* stream);

/* General linear layer on packed weights: Y[M,N] = A[M,K] * P (+ bias[N]) (+ resid[M,N]).  P is the forward
 * pack of W[N,K] (y = x W^T; Np = round16(N), col0 = 0) or the backward pack of W[N',K'] for dx = dy W
 * (then K = N', N = K' or a column slice starting at col0, Np = round16(K')+16).  K <= 4096 (above 1024 the
 * register-streamed tile form stages A in 1024-column chunks inside one workgroup); N is
 * unbounded (column groups).  Replaces nn.Linear / addmm + residual adds of the CDT block
 * (osrl/common/net.py:406-415,439-440, osrl/algorithms/cdt.py:96-141) and their input gradients. */
int osrl_linear(const float* A, int64_t lda, int32_t M, int32_t K, const float* P, int32_t Np, int32_t col0,
                int32_t N, const float* bias, const float* resid, int64_t ldr, float* Y, int64_t ldy, void* stream);
/* dynamic LDS per workgroup of that chunked form (K > 1024 where the big-M kernels do not take the shape) */
int64_t osrl_linear_kchunk_lds_bytes(void);
/* dynamic LDS per workgroup of a wide-path MLP layer launch with K inputs and N outputs (0: K outside 1..OSRL_MAX_WIDTH) */
int64_t osrl_mlp_wide_lds_bytes(int32_t K, int32_t N);
/* Refresh the packed copies of `n_entries` weights (entries in DEVICE memory).  Sizes in floats:
 * forward round16(in)*round16(out), backward round16(out)*(round16(in)+16).  max_elems = the largest
 * packed size among the entries (grid sizing).  Must run after every change of the canonical weights. */
int osrl_pack_weights(const float* src_flat, float* pf, float* pb, const osrl_pack_entry_t* d_entries,
                      int32_t n_entries, int32_t max_elems, void* stream);
/* The opt-in "bf16x3" form of osrl_linear (linear_split.hip; new, no counterpart in the reference): the same
 * Y[M,N] = A[M,K] * W^T (+ bias[N]) (+ resid[M,N]) with W[N,K] given as THREE bf16 planes (osrl_split_planes), each
 * [N,K] row-major, plane_stride elements apart (>= N*K, a multiple of 8).  Every fp32 value is the exact sum of three
 * bf16 pieces (truncation split); the six piece products that matter run on v_mfma_f32_32x32x16_bf16 and are summed in
 * fp32 in a fixed order (a function of K alone: same bits on every launch), the three dropped ones are <= 2^-23 |a||w|
 * per product -- fp32-class, NOT bit-equal to osrl_linear.  Any M (the row tail is masked).  Takes the shapes for which
 * osrl_linear_split_supported returns 1 (K % 32 == 0, N % 128 == 0); A and Wp 16-byte aligned, lda % 4 == 0; anything else
 * is -1 and the caller keeps osrl_linear.  The input gradient dX = dY W is the same call on the planes of W^T.
 * Non-finite inputs: the split of +-Inf is (Inf, NaN, NaN), so every output fed by an Inf or NaN element of A or W is
 * NaN (never a finite number; also where fp32 arithmetic would give +-Inf).  Values below 2^-110 in magnitude: their
 * bits under 2^-133 (bf16's smallest subnormal) are not representable in any piece and are dropped. */
int osrl_linear_split(const float* A, int64_t lda, int32_t M, int32_t K, const uint16_t* Wp, int64_t plane_stride,
                      int32_t N, const float* bias, const float* resid, int64_t ldr, float* Y, int64_t ldy, void* stream);
int osrl_linear_split_supported(int32_t M, int32_t K, int32_t N);   /* 1 / 0; no launch */
int64_t osrl_linear_split_lds_bytes(void);                            /* dynamic LDS per workgroup of that kernel */
/* Refresh the bf16 planes of `n_entries` canonical weights in ONE launch (entries in DEVICE memory, as for
 * osrl_pack_weights; offsets in bf16 ELEMENTS): f_off = where the three planes of W[out,in] go in planes_w, b_off = where
 * the three planes of W^T[in,out] go in planes_t (what dX reads); the planes of one matrix are out*in elements apart;
 * a negative offset or a NULL buffer skips that orientation.  max_elems = the largest out*in (grid sizing).
 * hipGraph-capturable.  Must run after every change of the canonical weights. */
int osrl_split_planes(const float* src_flat, uint16_t* planes_w, uint16_t* planes_t, const osrl_pack_entry_t* d_entries,
                      int32_t n_entries, int32_t max_elems, void* stream);
/* entries/items live in DEVICE memory (static plan): items[i] = {entry, o_tile, i_tile, 0} with
 * 64x64 tiles; slabs = [n_splits][slab_stride] partial gradients (deterministic split-K over rows). */
int osrl_mlp_backward_dw(const osrl_dw_entry_t* d_entries, const int32_t* d_items, int32_t n_items,
                         int32_t rows, int32_t n_splits, float* slabs, int64_t slab_stride, void* stream);
/* The same GEMMs on (16 * tile_blocks)^2 tiles (tile_blocks = 4 | 5) with a FLAT work list: d_work[4 i ..] =
 * (entry, out tile, in tile, split | n_splits << 16); every (tile, split) pair is one workgroup and writes slab `split`.
 * Lets the caller give tiles of unequal work unequal row splits and pick 80 x 80 tiles for 400-wide layers (25 column
 * blocks = 5 x 5: no ragged tiles).  Same per-element arithmetic as osrl_mlp_backward_dw. */
int osrl_mlp_backward_dw_tiles(const osrl_dw_entry_t* d_entries, const int32_t* d_work, int32_t n_work, int32_t rows,
                               int32_t tile_blocks, float* slabs, int64_t slab_stride, void* stream);
/* osrl_mlp_backward_dw_tiles AND the optimizer step of the group the gradients belong to, in ONE launch (new: the
 * reference runs loss.backward() and optimizer.step() as separate passes, cpq.py:131-133,149-151,196-198,218-220):
 * every (tile, split) workgroup stores its slab tile as above and signs in at its tile's arrival counter
 * (d_counters[d_tile_ids[i]], uint32, ZERO before the first launch; the last split to arrive re-arms it); that last
 * workgroup sums the tile's n_splits slabs in slab order and applies osrl_adam_step_packed's update (weight decay 0,
 * no gradient scale) to the tile's parameters: p, m, v, the Polyak target (tgt, may be NULL) and the packed copies
 * through map_f / map_b (may be NULL).  Same bits as the two launches it replaces.  Nobody waits inside the kernel (a
 * workgroup either is the last of its tile or leaves), so there is no residency requirement.  The work list must
 * cover every parameter of the group that has a gradient exactly once per split; d_tile_ids[i] is the same for the
 * n_splits items of a tile and different between tiles.  NOT for data-parallel steps (the all-reduce sits between dW
 * and the update there).  HOST struct. */
typedef struct {
  float *p, *m, *v, *tgt;            /* flat group buffers (tgt may be NULL) */
  const int32_t *map_f, *map_b;      /* osrl_adam_step_packed's maps (may be NULL) */
  float *pf, *pb, *tf;               /* packed copies (tf: packed Polyak target, may be NULL) */
  const osrl_step_state_t* st;       /* bias corrections / warm-up factor of the current step */
  float lr, beta1, beta2, eps, tau;
  int32_t pad_;
} osrl_dw_adam_t;
int osrl_mlp_backward_dw_tiles_adam(const osrl_dw_entry_t* d_entries, const int32_t* d_work, const int32_t* d_tile_ids,
                                    uint32_t* d_counters, int32_t n_work, int32_t rows, int32_t tile_blocks,
                                    float* slabs, int64_t slab_stride, const osrl_dw_adam_t* opt, void* stream);
/* The same contract for items given in units of 128 (out) x 64 (in) tiles that lie fully inside their dW (only
 * full tiles may be listed): one wave per tile and row split, 128-register accumulator tiles, one wave per SIMD -- the big-row-count (token matrix) variant; db of an entry is written by its it == 0 tiles.
 * Splits beyond a plan's own n_splits are never written (the caller keeps them zero).
 * The operands are read with 16-byte loads: dz / a of every listed entry 16-byte aligned, row strides % 4 == 0, and the
 * gradient slab 16-byte aligned with w_off % 4 == 0 (the caller checks: entries are device memory). */
int osrl_mlp_backward_dw_big(const osrl_dw_entry_t* d_entries, const int32_t* d_items, int32_t n_items, int32_t rows,
                             int32_t n_splits, float* slabs, int64_t slab_stride, void* stream);
/* The same contract for items in units of 256 (out) x 256 (in) tiles (out % 256 == 0, in % 256 == 0): one 8-wave
 * workgroup per tile and row split, the operands staged through LDS by DMA and shared by the eight waves.  rows % 16 == 0;
 * alignment as above.  db of an entry is written by its it == 0 tiles. */
int osrl_mlp_backward_dw_coop(const osrl_dw_entry_t* d_entries, const int32_t* d_items, int32_t n_items, int32_t rows,
                              int32_t n_splits, float* slabs, int64_t slab_stride, void* stream);

/* ---- optimizer (optim.hip): torch.optim.Adam/AdamW.step + _soft_update (cpq.py:107-113,232-238) ---- */
/* Advance the device step state (t += 1, bias corrections, LR-warmup factor).  If stats_cur/ring are
 * given, first commits the previous step's statistics into ring[((t-1) % ring_len)][n_stats] so that
 * the host can read logged values lazily instead of .item()-syncing every step. */
int osrl_step_tick(osrl_step_state_t* st, float beta1, float beta2, int32_t warmup, const float* stats_cur,
                   float* ring, int32_t n_stats, int32_t ring_len, void* stream);
/* The whole step prologue in ONE launch: osrl_step_tick + osrl_randn_fill (if noise != NULL) + osrl_replay_gather (if
 * n_fields > 0), with exactly their results -- the draws use step t+1, the value the tick is about to store; the last
 * workgroup to have read the old step performs the tick.  Replaces three dependent launches (and their launch gaps)
 * at the head of every train step. */
int osrl_step_begin(osrl_step_state_t* st, float beta1, float beta2, int32_t warmup, const float* stats_cur,
                    float* ring, int32_t n_stats, int32_t ring_len, float* noise, int64_t noise_n,
                    uint64_t noise_seed, uint32_t noise_stream, int32_t n_fields, const float* const* src,
                    float* const* dst, const int32_t* width, const float* scale, int64_t n_rows, int32_t batch,
                    uint64_t gather_seed, uint32_t gather_stream, void* stream);
/* The two calls above for TWO step states that take turns (software-pipelined train steps: step k+1's prologue runs while
 * step k's last optimizer launches still read step k's bias corrections, so consecutive steps cannot share one state).
 * `st` receives t = max(st->step, peer->step) + 1 and commits ITS OWN previous statistics (those of step st->step) to the
 * ring slot of that step; `peer` is only read.  peer == NULL: exactly osrl_step_tick / osrl_step_begin.  The reference has
 * no counterpart (its optimizer steps are host-serialised, cpq.py:294-313); same arithmetic per step as the plain calls. */
int osrl_step_tick_peer(osrl_step_state_t* st, const osrl_step_state_t* peer, float beta1, float beta2, int32_t warmup,
                        const float* stats_cur, float* ring, int32_t n_stats, int32_t ring_len, void* stream);
int osrl_step_begin_peer(osrl_step_state_t* st, const osrl_step_state_t* peer, float beta1, float beta2, int32_t warmup,
                         const float* stats_cur, float* ring, int32_t n_stats, int32_t ring_len, float* noise,
                         int64_t noise_n, uint64_t noise_seed, uint32_t noise_stream, int32_t n_fields,
                         const float* const* src, float* const* dst, const int32_t* width, const float* scale,
                         int64_t n_rows, int32_t batch, uint64_t gather_seed, uint32_t gather_stream, void* stream);
/* The two prologues with osrl_replay_gather_w's table (cum == NULL: exactly the calls above). */
int osrl_step_begin_w(osrl_step_state_t* st, float beta1, float beta2, int32_t warmup, const float* stats_cur,
                      float* ring, int32_t n_stats, int32_t ring_len, float* noise, int64_t noise_n,
                      uint64_t noise_seed, uint32_t noise_stream, int32_t n_fields, const float* const* src,
                      float* const* dst, const int32_t* width, const float* scale, int64_t n_rows, int32_t batch,
                      uint64_t gather_seed, uint32_t gather_stream, const uint64_t* cum, void* stream);
int osrl_step_begin_peer_w(osrl_step_state_t* st, const osrl_step_state_t* peer, float beta1, float beta2, int32_t warmup,
                           const float* stats_cur, float* ring, int32_t n_stats, int32_t ring_len, float* noise,
                           int64_t noise_n, uint64_t noise_seed, uint32_t noise_stream, int32_t n_fields,
                           const float* const* src, float* const* dst, const int32_t* width, const float* scale,
                           int64_t n_rows, int32_t batch, uint64_t gather_seed, uint32_t gather_stream,
                           const uint64_t* cum, void* stream);
/* The prologue over a store that grows (osrl_replay_gather_n; n_rows_dev == NULL: exactly osrl_step_begin_peer_w). */
int osrl_step_begin_peer_n(osrl_step_state_t* st, const osrl_step_state_t* peer, float beta1, float beta2, int32_t warmup,
                           const float* stats_cur, float* ring, int32_t n_stats, int32_t ring_len, float* noise,
                           int64_t noise_n, uint64_t noise_seed, uint32_t noise_stream, int32_t n_fields,
                           const float* const* src, float* const* dst, const int32_t* width, const float* scale,
                           int64_t n_rows, int32_t batch, uint64_t gather_seed, uint32_t gather_stream,
                           const uint64_t* cum, const int64_t* n_rows_dev, void* stream);
/* g = sum_s slabs[s][i] (* *gscale if gscale != NULL); AdamW decay if weight_decay != 0;
 * then tgt = tau*p + (1-tau)*tgt if tgt != NULL.  n and slab_stride must be multiples of 4. */
int osrl_adam_step(float* p, float* m, float* v, float* tgt, const float* slabs, int32_t n_splits,
                   int64_t slab_stride, int64_t n, float lr, float beta1, float beta2, float eps,
                   float weight_decay, float tau, const float* gscale, const osrl_step_state_t* st,
                   void* stream);
/* Same step, and the packed weight copies (osrl_pack_weights layouts) are refreshed in the same pass:
 * map_f[i] / map_b[i] = float index of flat parameter i inside pf / pb (-1 = not a packed weight; map_b may be
 * NULL); tf (may be NULL) receives the Polyak target at map_f.  Padding of the packed buffers is not touched. */
int osrl_adam_step_packed(float* p, float* m, float* v, float* tgt, const float* slabs, int32_t n_splits,
                          int64_t slab_stride, int64_t n, float lr, float beta1, float beta2, float eps,
                          float weight_decay, float tau, const float* gscale, const osrl_step_state_t* st,
                          const int32_t* map_f, const int32_t* map_b, float* pf, float* pb, float* tf,
                          void* stream);
/* The Polyak step alone: tgt = tau p + (1 - tau) tgt, and tf[map_f[i]] = the new target where map_f[i] >= 0 (map_f / tf may
 * be NULL) -- the bits osrl_adam_step(_packed) leaves when it carries the step.  For a plan whose last reader of the OLD
 * targets runs after the group's optimizer step (reference order: every loss of cpq.py:294-313 reads the targets of the
 * step's start, sync_weight() comes last).  n a multiple of 4. */
int osrl_polyak(const float* p, float* tgt, int64_t n, float tau, const int32_t* map_f, float* tf, void* stream);
/* flat[i] = sum_s slabs[s][i]  (pre-reduction before an RCCL all-reduce in the data-parallel path) */
int osrl_reduce_slabs(float* flat, const float* slabs, int32_t n_splits, int64_t slab_stride, int64_t n,
                      void* stream);
/* The same sum with a row-split count per 1024-float chunk of the flat gradient (counts: device bytes, ceil(n / 1024) of
 * them, each >= 1): a group whose ranges were written by plans with different split counts (CDT: cdt.py:396-400 needs the
 * summed gradient for clip_grad_norm_) reads only the slabs that hold something.  Same bits as osrl_reduce_slabs with the
 * largest count, since the slabs beyond a range's own count are zero. */
int osrl_reduce_slabs_counts(float* flat, const float* slabs, const uint8_t* counts, int64_t slab_stride, int64_t n,
                             void* stream);

/* ---- device-resident argument blocks for the launches of a captured step (csrc/argmem.h) --------------------
 * New (nothing in the reference to mirror: torch passes kernel arguments through the runtime).  The fused-MLP
 * launches carry 1.2-2.4 KB descriptors by value; where the HIP runtime keeps kernel arguments in HOST memory (no
 * large BAR, or HIP_FORCE_DEV_KERNARG=0) every wave fetches them over PCIe and a train step loses ~20 %.  A step
 * engine's launches are static, so the caller may keep the descriptors in HBM instead:
 *   1. osrl_args_begin(staging, NULL, cap, 0, 1)   record: run the step once (eagerly); every fused-MLP launch also
 *      copies its descriptor into `staging` (host memory, identical blocks once);  osrl_args_end(&used, ...);
 *   2. copy staging[0:used] to device memory `dev` (any hipMemcpy);
 *   3. osrl_args_begin(staging, dev, cap, used, 2)  replay: run the step again (typically under hipGraph capture);
 *      a launch whose descriptor is found in the staging buffer BY CONTENT starts the kernel variant that reads it
 *      from `dev`; anything else is launched by value as always (counted in n_misses);  osrl_args_end(...).
 * The context belongs to the calling thread; without it nothing changes.  `dev` must outlive the captured graph.
 * Returns 0, -1 on bad arguments / no open context, -2 when a context is already open on this thread. */
int osrl_args_begin(void* host_staging, const void* dev_copy, int64_t capacity, int64_t used, int32_t mode);
int osrl_args_end(int64_t* used, int32_t* n_blocks, int32_t* n_hits, int32_t* n_misses);

/* ---- RNG + replay (rng.hip): torch.randn / TransitionDataset sampling (dataset.py:832-847) ---- */
/* out[i] ~ N(0,1): Philox4x32-10 keyed by seed, counter = (i/4, st->step, stream_id), Box-Muller. */
int osrl_randn_fill(float* out, int64_t n, uint64_t seed, uint32_t stream_id, const osrl_step_state_t* st,
                    void* stream);
/* idx[b] ~ U{0..n_rows-1} (with replacement) and gather of `n_fields` (<= 8) row-major fp32 tables:
 * dst[f][b, :width[f]] = src[f][idx[b], :width[f]] * scale[f].  src/dst/width/scale are HOST arrays
 * of device pointers / ints / floats (copied into the launch). idx_out (device int32[batch]) optional. */
int osrl_replay_gather(int32_t n_fields, const float* const* src, float* const* dst, const int32_t* width,
                       const float* scale, int64_t n_rows, int32_t batch, int32_t* idx_out, uint64_t seed,
                       uint32_t stream_id, const osrl_step_state_t* st, void* stream);
/* Weighted transition sampling (ReplayStore.set_sample_prob; the reference draws uniformly, dataset.py:846, and offers
 * only the hard filters of process_bc_dataset).  `weights`: one non-negative finite fp64 value per row, positive sum.
 *   The table.  cum[i] (device uint64[n_rows]) = floor(2^64 * S_i / S_n) saturated at 2^64 - 1, S_i the fp64 inclusive
 *     prefix sum of the weights in index order: S_i = O_b + (T_j + L_e), with L_e the running sum inside a thread's 16
 *     consecutive rows, T_j the running sum of the thread totals inside a workgroup's 4096 rows and O_b the running sum
 *     of the workgroup totals, each of the three chains added left to right from 0 -- one fixed association, so two
 *     builds give the same bits, S is non-decreasing, and a zero-weight row has exactly its predecessor's entry (0 for
 *     leading rows).  cum[n_rows - 1] = 2^64 - 1 always.  A weight below 2^-64 of the total (2^-53 of it near the end of the
 *     table, where fp64 resolves no finer) may share its predecessor's entry and is then never drawn.  Negative and NaN
 *     weights count as 0; a sum that is not positive gives the table that always draws row 0.
 *   The draw.  Row b's word is the one the uniform draw maps: u = (r.x << 32) | r.y of
 *     philox4x32_10({b, 0x5eed, step, stream_id}, seed).  idx[b] = the FIRST i with cum[i] > min(u, 2^64 - 2): the word
 *     2^64 - 1, which no entry exceeds, draws what 2^64 - 2 draws.  So a zero-weight row is never drawn, whatever the
 *     word (leading rows hold 0, later ones repeat their predecessor and are never the first), and the index depends on
 *     (table, word) only.  The lanes that hold a row search together: 64 (32 in osrl_mlp_regress_step) evenly spaced
 *     probes and a ballot per round, ceil(log_65 n) (log_33) dependent loads.
 *   cum == NULL: the uniform draw, bit for bit the calls without the table.
 * osrl_weights_cum_u64 builds the table (3 launches, n <= 2^28, rewritten in place: a captured graph that holds the address
 * draws from the new weights at its next replay); ws: osrl_weights_cum_u64_ws_elems(n) doubles of device scratch. */
int64_t osrl_weights_cum_u64_ws_elems(int64_t n);
int osrl_weights_cum_u64(const double* weights, int64_t n, uint64_t* cum, double* ws, void* stream);
int osrl_replay_gather_w(int32_t n_fields, const float* const* src, float* const* dst, const int32_t* width,
                         const float* scale, int64_t n_rows, int32_t batch, int32_t* idx_out, uint64_t seed,
                         uint32_t stream_id, const osrl_step_state_t* st, const uint64_t* cum, void* stream);
/* A store that grows (ReplayStore(capacity=); the reference's datasets are fixed, dataset.py:790-847).  The tables (and
 * cum) are allocated for n_rows = the capacity; n_rows_dev (device int64, one word) holds the live row count.  Every row
 * of the batch reads the word once and draws over n = min(max(*n_rows_dev, 1), n_rows): the uniform draw is
 * umul64hi(u, n), the weighted one the first i in [0, n) with cum[i] > the word of osrl_replay_gather_w, over the first
 * n entries.  Whatever the word holds, the index lies inside [0, n_rows).  The kernels only read the word: the caller
 * writes it on the stream between launches, so a captured graph that holds its address follows the store at its next
 * replay.  n_rows_dev == NULL: exactly osrl_replay_gather_w, bit for bit. */
int osrl_replay_gather_n(int32_t n_fields, const float* const* src, float* const* dst, const int32_t* width,
                         const float* scale, int64_t n_rows, int32_t batch, int32_t* idx_out, uint64_t seed,
                         uint32_t stream_id, const osrl_step_state_t* st, const uint64_t* cum,
                         const int64_t* n_rows_dev, void* stream);

/* CDT minibatch source -- SequenceDataset.__iter__/__prepare_sample (dataset.py:749-787) on device: per sample
 * draw a trajectory (inverse CDF of `cdf`, or uniform when NULL) and a start ~ U{0..len-1}, slice seq_len steps
 * of the concatenated trajectory tables (clipped at the trajectory end), zero-pad the tail, emit mask,
 * time_steps = start + arange(T), returns*reward_scale, cost_returns*cost_scale, episode_cost =
 * cost_returns[first step]*cost_scale.  ONE descriptor (HOST struct, copied into the launch) and one entry point: an
 * absent feature is a NULL field.  The seven tables and the eight outputs are required. */
typedef struct {
  const float *obs, *act, *returns, *cost_returns, *costs; /* concatenated trajectories [total rows, .] */
  const int64_t* traj_start;
  const int32_t* traj_len;
  const float* cdf; /* inclusive cumulative trajectory-sampling probabilities, or NULL = uniform */
  /* optional, [total rows]: inclusive cumulative start-index probabilities inside each trajectory
   * (SequenceDataset(start_sampling=True), dataset.py:742-744,781-783; osrl_start_index_prob) -- NULL = uniform starts */
  const float* start_cdf;
  const int32_t* idx_in; /* optional, [B,2]: (trajectory, start) pairs given by the caller instead of drawn (fixed evaluation windows) */
  /* A store that grows: traj_start / traj_len / cdf are allocated for n_traj = the capacity, n_traj_dev (device int32,
   * one word, only read here) holds the live trajectory count, and the uniform draw and the cdf bisection run over
   * min(max(*n_traj_dev, 1), n_traj) trajectories.  n_traj_dev == NULL: a fixed store, the draw over n_traj. */
  const int32_t* n_traj_dev;
  float *o_states, *o_actions, *o_returns, *o_cost_returns;
  int64_t* o_time_steps;
  float *o_mask, *o_episode_cost, *o_costs;
  int32_t* idx_out; /* optional, [B,2]: receives (trajectory, start) per sample */
  uint64_t seed;
  int32_t n_traj, B, T, od, ad;
  float reward_scale, cost_scale;
  uint32_t stream_id;
} osrl_seq_gather_t;
int osrl_seq_window_gather(const osrl_seq_gather_t* g, const osrl_step_state_t* st /* NULL: step 0 */, void* stream);

/* A store that evicts (SequenceStore evict="oldest", seq_ring.hip): drop the n_drop oldest of the n_live trajectories.
 * Entries [n_drop, n_live) of traj_start, traj_len and (if given) traj_w move to [0, n_live - n_drop) IN PLACE, the
 * vacated slots [n_live - n_drop, n_live) are zeroed, entries past n_live are not touched, and *n_traj_dev (the live
 * word osrl_seq_window_gather reads) becomes n_live - n_drop.  One launch of one workgroup that walks the tables in
 * ascending passes (load a pass, barrier, store it), so source and destination may overlap; no workspace, capturable.
 * 0 <= n_drop <= n_live <= 2^20; -1 (nothing launched) otherwise or on a NULL traj_start / traj_len / n_traj_dev. */
typedef struct {
  int64_t* traj_start;
  int32_t* traj_len;
  double* traj_w; /* optional per-trajectory weights (set_sample_prob), NULL = none */
  int32_t* n_traj_dev;
  int32_t n_live, n_drop;
} osrl_seq_evict_t;
int osrl_seq_evict_front(const osrl_seq_evict_t* e, void* stream);

/* ---- glue (glue.hip): the elementwise / reduction tails of the loss functions ----
 * `rows_global` (0 = rows) is the data-parallel global batch used in every 1/B normalisation.
 * `stat` pointers are device floats (logged statistics), may be NULL. */
/* SquashedGaussianMLPActor tail net.py:176-201: head=[rows,2*ad]=(mu|log_std_raw);
 * u = mu + exp(clamp(ls,-20,2))*eps (eps NULL => deterministic), a = max_action*tanh(u).
 * Outputs (each may be NULL): a[rows,ad], tanh_u[rows,ad], logp[rows]. */
int osrl_gauss_head(const float* head, const float* eps, int32_t rows, int32_t ad, float max_action,
                    float* a, float* tanh_u, float* logp, void* stream);
/* d head from d a (autograd of the tail above); da_nets = [n_nets][rows,ad] is summed over nets. */
int osrl_gauss_head_bwd(const float* head, const float* eps, const float* tanh_u, const float* da_nets,
                        int32_t n_nets, int32_t rows, int32_t ad, float max_action, float* dhead,
                        void* stream);
/* pi_dist.sample([N]) cpq.py:166-169: out[j*rows+b,:] = mu[b] + std[b]*eps[j,b,:]  (pre-tanh) */
int osrl_gauss_ood_sample(const float* head, const float* eps, int32_t n_samples, int32_t rows, int32_t ad,
                          float* out, void* stream);
/* VAE latent net.py:323-327: head=[rows,2L]=(mean|log_std_raw) -> z = mean + exp(clamp(ls,-4,15))*eps */
int osrl_vae_latent(const float* head, const float* eps, int32_t rows, int32_t L, float* z, void* stream);
/* vae_loss cpq.py:125-129 == bcql.py:122-126: stat = mse(u, act) + beta*KL(head); du = d loss / d u. */
int osrl_vae_loss(const float* u, const float* act, const float* head, int32_t rows, int32_t ad, int32_t L,
                  float beta, int32_t rows_global, float* du, float* stat, void* stream);
/* d head of the VAE latent given dz = d loss / d z from the decoder backward (+ the KL term). */
int osrl_vae_latent_bwd(const float* head, const float* eps, const float* dz, int32_t rows, int32_t L,
                        float beta, int32_t rows_global, float* dhead, void* stream);
/* per-row mean over the latent of the KL term (cpq.py:181-182): kl[r] */
int osrl_vae_kl_rows(const float* head, int32_t rows, int32_t L, float* kl, void* stream);
/* torch.quantile(x, q) (linear interpolation) by an exact 4-pass radix select; out[0] = quantile. */
int osrl_quantile(const float* x, int64_t n, float q, float* out, void* stream);

/* CPQ critic target + loss gradient (cpq.py:145-148, net.py:240-242).
 * q_old/qc_old/q are [n][rows] net-major outputs. dq[e][rows] = 2(q_e-backup)/B; stat = sum_e mse. */
int osrl_cpq_critic_loss(const float* q_old, int32_t n_q_old, const float* qc_old, int32_t n_qc_old,
                         const float* q, int32_t n_q, const float* rew, const float* done, int32_t rows,
                         float gamma, float q_thres, int32_t rows_global, float* dq, float* stat, void* stream);
/* The same quantile for large n (the all-gathered KL rows of data-parallel CPQ: world * N * B values) as a grid: four
 * multi-workgroup histogram passes + a successor search + a finish launch instead of one streaming workgroup (200 us
 * at n = 163840).  ws: OSRL_QUANTILE_WS uint32 of device scratch, all zero before the first call; every call leaves it
 * zeroed again.  Same result bits as osrl_quantile. */
#define OSRL_QUANTILE_WS 1032
int osrl_quantile_ws(const float* x, int64_t n, float q, uint32_t* ws, float* out, void* stream);
/* out[0] = mean over the (global) batch of qc_ood = ((KL >= quantile) * min_e qc_sampled).mean(0)
 * (cpq.py:184,187); under data parallelism this rank's share, to be all-reduced(SUM). */
int osrl_cpq_ood_mean(const float* qc_sampled, int32_t n_qc_old, const float* kl, const float* quantile,
                      int32_t n_samples, int32_t rows, int32_t rows_global, float* out, void* stream);
/* osrl_quantile(kl, n_samples*rows, q) + osrl_cpq_ood_mean in ONE launch (cpq.py:183-184,187; single-GPU step):
 * quant_out[0] = the quantile, out[0] = the OOD mean; same bits as the two calls.  n_samples*rows <= 32768 (-2). */
int osrl_cpq_ood_stat(const float* qc_sampled, int32_t n_qc_old, const float* kl, float q, int32_t n_samples,
                      int32_t rows, int32_t rows_global, float* quant_out, float* out, void* stream);
/* cpq.py:183-184 as a ROW SET instead of a mask: qc_ood = ((KL >= quantile) * qc_sampled).mean(0) multiplies three
 * quarters of the N*B target-cost-critic outputs by zero; with the rows that count known BEFORE those networks run, they
 * run on that quarter only (osrl_rows_t.row_list / n_rows_dev).
 *   osrl_cpq_ood_select: quantile = *quantile_in if given, else the q-quantile of kl[0..n) (torch.quantile 'linear',
 *     n <= 32768: -2 otherwise); list[0..count) = the indices i, ascending, with kl[i] >= quantile; count[0], quant_out[0].
 *   osrl_cpq_ood_sum: out[0] = scale * sum_{r < min(*count, cap)} min_e qc_sel[e * cap + r]   (scale = 1 / (n_samples *
 *     rows_global): the mean over the batch of the mean over the samples; fixed summation order).
 * Equal to osrl_cpq_ood_stat on the full rows up to the order of the sum (and to a non-finite critic output on a row
 * OUTSIDE the set, which the reference's multiplication by zero would turn into NaN). */
int osrl_cpq_ood_select(const float* kl, const float* quantile_in, float q, int32_t n, float* quant_out, int32_t* list,
                        int32_t* count, void* stream);
int osrl_cpq_ood_sum(const float* qc_sel, int32_t n_qc, int32_t cap, const int32_t* count, float scale, float* out,
                     void* stream);
/* CPQ cost-critic loss (cpq.py:161,186-199): backup = c + gamma*min qc_old; dq = 2(qc-backup)/B;
 * log_alpha (device scalar) ascends with the GLOBAL ood_mean (device scalar) and is clamped to +-5;
 * stat[0] = loss, stat[1] = exp(log_alpha) after the update.  stat_share = 1/world_size scales the
 * batch-global terms of the statistics so that an all-reduce(SUM) of per-rank stats is exact. */
int osrl_cpq_cost_loss(const float* qc_old_next, int32_t n_qc_old, const float* qc, int32_t n_qc,
                       const float* ood_mean, const float* cost, int32_t rows, float gamma, float qc_thres,
                       float alpha_lr, int32_t rows_global, float stat_share, float* log_alpha, float* dq,
                       float* stat, void* stream);
/* ood_mean == NULL in osrl_cpq_cost_loss defers the dual step: stat[0] = the MSE part only and log_alpha is left
 * alone (the gradient dq never depends on ood_mean, cpq.py:186-199 -- qc_ood is under no_grad and log_alpha has no
 * grad); osrl_cpq_alpha_step then applies it once the GLOBAL ood_mean is known: stat[0] -= share*exp(la)*(ood-thres),
 * log_alpha += alpha_lr*exp(la)*(thres - ood), clamp +-5, stat[1] = share*exp(log_alpha).  Data parallelism uses
 * this to fold the ood_mean reduction into the gradient all-reduce of the phase. */
int osrl_cpq_alpha_step(const float* ood_mean, float qc_thres, float alpha_lr, float stat_share, float* log_alpha,
                        float* stat, void* stream);
/* Single-GPU fusion of osrl_cpq_ood_mean + osrl_cpq_cost_loss (cpq.py:184-199): the OOD mean is computed inside
 * the loss launch (and written to ood_mean_out); no batch-global reduction can sit between the two. */
int osrl_cpq_cost_loss_ood(const float* qc_sampled, int32_t n_qc_sampled, const float* kl, const float* quantile,
                           int32_t n_samples, const float* qc_old_next, int32_t n_qc_old, const float* qc,
                           int32_t n_qc, float* ood_mean_out, const float* cost, int32_t rows, float gamma,
                           float qc_thres, float alpha_lr, float* log_alpha, float* dq, float* stat, void* stream);
/* CPQ actor loss (cpq.py:210-212): loss = -mean(1[min qc <= thres] * min q); dq routed to arg-min net. */
int osrl_cpq_actor_loss(const float* q, int32_t n_q, const float* qc, int32_t n_qc, int32_t rows,
                        float q_thres, int32_t rows_global, float* dq, float* stat, void* stream);
/* F.mse_loss (bc.py:46-47): stat = mean((u-target)^2) over n elements; du = 2(u-target)/n_global */
int osrl_mse_loss(const float* u, const float* target, int64_t n, int64_t n_global, float* du, float* stat,
                  void* stream);

/* Value read-out of fitted Q evaluation: acc[e] += sum_r q[e * rows + r] in fp64 (q = [n_nets, rows] critic outputs, acc =
 * n_nets device doubles that the caller zeroes once and then accumulates into chunk by chunk).  ONE workgroup, one fixed
 * summation order per net (each lane a contiguous chunk of rows, lanes by the butterfly, waves in order), so a value is
 * reproducible bit for bit; n_nets <= OSRL_MAX_NETS, rows >= 1. */
int osrl_fqe_value_sums(const float* q, int32_t n_nets, int32_t rows, double* acc, void* stream);
/* in-place clamp: the `.clamp(-0.5, 0.5)` of VAE.decode's latent draw (net.py:334-335) */
int osrl_clamp(float* x, int64_t n, float lo, float hi, void* stream);
/* BCQ-Lag perturbation tail net.py:61-62: a = clamp(dec + phi*max_a*t, +-max_a) */
int osrl_bcq_perturb(const float* dec, const float* t, int32_t rows, int32_t ad, float phi, float max_action,
                     float* a, void* stream);
/* d t of the perturbation actor from d a (da_nets [n_nets][rows,ad] summed), through the clamp */
int osrl_bcq_perturb_bwd(const float* dec, const float* t, const float* da_nets, int32_t n_nets, int32_t rows,
                         int32_t ad, float phi, float max_action, float* dt, void* stream);
/* BCQ-Lag target (bcql.py:144-150): q_t[e][rows*N] (first n1 = q1 nets, then n2 = q2 nets), row b*N+j ->
 * backup[b] = base[b] + gamma*(1-done[b])*max_j(lmbda*min(q1,q2)+(1-lmbda)*max(q1,q2)); then
 * dq[e][b] = 2*(q_on[e][b]-backup[b])/B, stat = sum_e mse.  done may be NULL (cost critic, bcql.py:172). */
int osrl_bcq_critic_loss(const float* q_t, int32_t n1, int32_t n2, int32_t n_samples, const float* q_on,
                         int32_t n_on, const float* base, const float* done, int32_t rows, float gamma,
                         float lmbda, int32_t rows_global, float* dq, float* stat, void* stream);
/* The two batch-sum losses on a grid of <= 64 workgroups (for batches beyond ~2048 rows, where one workgroup walking the
 * batch alone costs 35-45 us): same values per row, the logged statistic is the sum of per-workgroup partials added in
 * workgroup order by the last workgroup to arrive (deterministic; no floating-point atomics).  ws: OSRL_LOSS_WS floats
 * of device memory, zeroed once before first use, private to one call site while a launch is in flight. */
#define OSRL_LOSS_WS 132
int osrl_bcq_critic_loss_ws(const float* q_t, int32_t n1, int32_t n2, int32_t n_samples, const float* q_on, int32_t n_on,
                            const float* base, const float* done, int32_t rows, float gamma, float lmbda,
                            int32_t rows_global, float* dq, float* stat, float* ws, void* stream);
int osrl_vae_loss_ws(const float* u, const float* act, const float* head, int32_t rows, int32_t ad, int32_t L, float beta,
                     int32_t rows_global, float* du, float* stat, float* ws, void* stream);
/* BCQ-Lag actor loss (bcql.py:190-198 + PID net.py:376-387).  q/qc = [n1+n2][rows] (q1 nets then q2 nets).
 * pid = device {error_old, error_integral}; stat: [0]=loss [1]=qc_penalty [2]=multiplier.
 * Data parallel: global_means = all-reduced {mean q_pi, mean qc_pi} from osrl_bcq_actor_sums (NULL = compute
 * locally), stat_share = 1/world. */
int osrl_bcq_actor_sums(const float* q, int32_t nq1, int32_t nq2, const float* qc, int32_t nc1, int32_t nc2,
                        int32_t rows, int32_t rows_global, float* out, void* stream);
int osrl_bcq_actor_loss(const float* q, int32_t nq1, int32_t nq2, const float* qc, int32_t nc1, int32_t nc2,
                        int32_t rows, float qc_thres, float KP, float KI, float KD, int32_t rows_global,
                        const float* global_means, float stat_share, float* pid, float* dq, float* dqc, float* stat,
                        void* stream);

/* ---- CDT (cdt.hip): the non-GEMM pieces of the Constrained Decision Transformer step ---- */
/* Token embeddings + timestep embedding, interleave and emb LayerNorm (cdt.py:178-222).  Tokens per timestep, in
 * order: [return if use_rew] [cost if use_cost] state action (R = 2..4); prefix != 0: one more token leads each
 * sequence, Linear(1,E) of episode_cost[b] (cdt.py:207-218); timestep_emb == NULL: time_emb = False.  S = R*T + prefix.
 * Outputs: seq[B*S,E] (pre-LN), x0[B*S,E], stats[B*S,2] = (mean, rstd), ctg_t[B*T] = the (optionally 50 - x
 * transformed, cdt.py:78-81) cost-to-go fed to cost_emb.  Pointers of absent tokens may be NULL. */
int osrl_cdt_embed_ln(const float* states, const float* actions, const float* returns, const float* costs_to_go,
                      const float* episode_cost, const int64_t* time_steps, const float* Ws, const float* bs,
                      const float* Wa, const float* ba, const float* Wc, const float* bc, const float* Wr,
                      const float* br, const float* Wp, const float* bp, const float* timestep_emb, const float* ln_g,
                      const float* ln_b, int32_t B, int32_t T, int32_t od, int32_t ad, int32_t E,
                      int32_t cost_transform, int32_t use_rew, int32_t use_cost, int32_t prefix, float* seq, float* x0,
                      float* stats, float* ctg_t, void* stream);
/* nn.LayerNorm (eps 1e-5) of x (+ delta): y = LN(x + delta); xout = x + delta if non-NULL; stats = (mean, rstd). */
int osrl_layernorm_fwd(const float* x, const float* delta, const float* gamma, const float* beta, float* xout,
                       float* y, float* stats, int32_t M, int32_t E, void* stream);
/* LayerNorm backward: dx = LN'(dy) (+ dres); dgamma/dbeta summed (fixed order, via partial_ws [n_parts, 2E]) into
 * slab[g_off..], slab[b_off..]. */
int osrl_layernorm_bwd(const float* dy, const float* x, const float* stats, const float* gamma, const float* dres,
                       float* dx, float* partial_ws, int32_t n_parts, int32_t M, int32_t E, float* slab,
                       int64_t g_off, int64_t b_off, void* stream);
/* The same two calls with the nn.Dropout of the residual branch folded in (net.py:414,439; round 3): forward applies
 * the keep-multiplier of `drop` to `delta` on the way in (== osrl_dropout(delta) then osrl_layernorm_fwd, bit for bit;
 * drop NULL or p <= 0: the plain call); backward also writes dx_dropped = dx * keep-multiplier of `drop` (the gradient
 * that enters the residual branch whose output fed this LayerNorm's input: == osrl_dropout on dx). */
/* slab == NULL in the two backward calls: the per-workgroup partials of (dgamma | dbeta) stay in partial_ws
 * ([n_parts, 2E]) and the caller sums them later -- osrl_layernorm_param_reduce does it for up to 16 LayerNorms in ONE
 * launch (site k: partials at partial_ws + k * ws_stride, results at slab[g_offs[k] ..], slab[b_offs[k] ..]; g_offs /
 * b_offs are HOST arrays).  Same bits as the per-call reduction (net.py:402-403,427,440 under autograd). */
int osrl_layernorm_param_reduce(const float* partial_ws, int64_t ws_stride, int32_t n_sites, int32_t n_parts, int32_t E,
                                float* slab, const int64_t* g_offs, const int64_t* b_offs, void* stream);
int osrl_layernorm_fwd_drop(const float* x, const float* delta, const osrl_dropout_t* drop, const float* gamma,
                            const float* beta, float* xout, float* y, float* stats, int32_t M, int32_t E,
                            void* stream);
int osrl_layernorm_bwd_drop(const float* dy, const float* x, const float* stats, const float* gamma, const float* dres,
                            float* dx, float* dx_dropped, const osrl_dropout_t* drop, float* partial_ws, int32_t n_parts,
                            int32_t M, int32_t E, float* slab, int64_t g_off, int64_t b_off, void* stream);
/* nn.MultiheadAttention core with the block's causal mask and key padding (net.py:417-435): qkv [B,S,3E] (q|k|v,
 * heads split the E axis contiguously), mask [B, (S-prefix)/rep] (1 = valid timestep, each repeated rep times along S;
 * prefix = 1: token 0 is the cost-prefix token, masked like timestep 0, cdt.py:216-218). */
int osrl_attention_fwd(const float* qkv, const float* mask, int32_t B, int32_t S, int32_t E, int32_t H, int32_t rep,
                       int32_t prefix, const osrl_dropout_t* drop, float* o, void* stream);
int osrl_attention_bwd(const float* qkv, const float* mask, const float* dout, int32_t B, int32_t S, int32_t E,
                       int32_t H, int32_t rep, int32_t prefix, const osrl_dropout_t* drop, float* dqkv, void* stream);
/* The same pair with the attention-probability dropout's keep decisions handed from the forward launch to the backward
 * launch instead of being regenerated there (head widths E / H = 16 or 32; net.py:406-409 -- torch keeps its dropout mask
 * for autograd the same way).  `keep`: caller-allocated, osrl_attention_keep_bytes(B, S, E, H) bytes (0 = shape not
 * supported: pass NULL), one nibble of four key decisions per byte; written by _fwd_keep when drop is active, read by
 * _bwd_keep of the SAME step.  The decisions are the Philox words' tests either way: results are bit-identical to the plain
 * pair, which the NULL form is. */
int64_t osrl_attention_keep_bytes(int32_t B, int32_t S, int32_t E, int32_t H);
int osrl_attention_fwd_keep(const float* qkv, const float* mask, int32_t B, int32_t S, int32_t E, int32_t H, int32_t rep,
                            int32_t prefix, const osrl_dropout_t* drop, float* o, unsigned char* keep, void* stream);
int osrl_attention_bwd_keep(const float* qkv, const float* mask, const float* dout, int32_t B, int32_t S, int32_t E,
                            int32_t H, int32_t rep, int32_t prefix, const osrl_dropout_t* drop, float* dqkv,
                            const unsigned char* keep, void* stream);
/* The same function for long sequences and wide heads: S <= 1024 tokens, head_dim = E / H <= 128 (any width; zero padded
 * to 16 / 32 / 64 / 128 inside).  Tiled kernels: 64-key tiles streamed through LDS with an online softmax, deterministic
 * (dQ by query tiles, dK / dV by key tiles, no atomics), the same dropout decisions as the pair above.
 * osrl_attention_ws_bytes(B, S, E, H) = 0 where osrl_attention_fwd / _bwd take the shape (S <= 128, head_dim <= 64);
 * otherwise, like osrl_attention_tiled_ws_bytes (which answers for every shape the _ws pair takes, 0 = not taken), it is
 * 4 * B * H * S: the size of `ws` of the backward AND of `lse`.  _fwd_ws writes o [B,S,E] and, when lse != NULL, the
 * per-row softmax statistics lse [B*H, S] (log2 domain of the scaled scores; +inf for a row without a valid key) that
 * _bwd_ws reads beside the forward's o (D_i = rowsum(dO o O) goes to ws).  lse = NULL: inference. */
int64_t osrl_attention_ws_bytes(int32_t B, int32_t S, int32_t E, int32_t H);
int64_t osrl_attention_tiled_ws_bytes(int32_t B, int32_t S, int32_t E, int32_t H);
/* dynamic LDS per workgroup of the tiled kernels at a head width: pass 0 forward, 1 dQ, 2 dK / dV (0 = not taken) */
int64_t osrl_attention_tiled_lds_bytes(int32_t head_dim, int32_t pass);
int osrl_attention_fwd_ws(const float* qkv, const float* mask, int32_t B, int32_t S, int32_t E, int32_t H, int32_t rep,
                          int32_t prefix, const osrl_dropout_t* drop, float* o, float* lse, void* stream);
int osrl_attention_bwd_ws(const float* qkv, const float* mask, const float* dout, int32_t B, int32_t S, int32_t E,
                          int32_t H, int32_t rep, int32_t prefix, const osrl_dropout_t* drop, const float* o,
                          const float* lse, float* ws, float* dqkv, void* stream);
/* nn.Dropout in training mode (cdt.py:87,222 embedding; net.py:404,439 residual; net.py:414 MLP tail):
 * y[i] = x[i] * keep_i / (1-p), may run in place.  keep_i is a pure function of (seed, st->step, site, i)
 * (Philox4x32-10), so calling it again on the incoming gradient IS the backward pass; nothing is stored.
 * `drop` of the attention entry points is the attention-probability dropout of nn.MultiheadAttention
 * (net.py:406-409), NULL or p = 0 = off; its logical mask layout is [B*H, S, Sp] (Sp = S rounded up to 16) with element
 * (bh*S + i)*Sp + j <-> P[bh][i][j], so osrl_dropout on a ones tensor of that size exports it. */
int osrl_dropout(const float* x, float* y, int64_t n, const osrl_dropout_t* drop, void* stream);
/* nn.GELU() (exact erf) and its derivative; n a multiple of 4 */
int osrl_gelu_fwd(const float* x, float* y, int64_t n, void* stream);
int osrl_gelu_bwd(const float* dy, const float* x, float* dx, int64_t n, void* stream);
/* CDTTrainer losses (cdt.py:357-394): head = (mu|log_std)[BT,2ad] (stochastic) or action prediction [BT,ad];
 * writes d head / d logits / d state_pred and stat[0..8] = nll, ent, ent_reg, all_loss, act_loss, cost_loss,
 * cost_acc, state_loss, train_lr; ent_out[0] = entropy (input of the temperature step).
 * ws (optional, >= 8 * ceil(B*T / 1024) floats) together with `counts`: one workgroup per 1024 tokens + an ordered
 * sum of their partials instead of one workgroup for the whole batch. */
int osrl_cdt_loss(const float* head, const float* logits, const float* state_pred, const float* actions,
                  const float* states, const float* mask, const float* costs, int32_t B, int32_t T, int32_t od,
                  int32_t ad, int32_t stochastic, int32_t no_entropy, const float* log_temperature, float cost_w,
                  float state_w, float lr, int32_t warmup, const osrl_step_state_t* st, const float* counts,
                  int32_t world, float* dhead, float* dlogits, float* dsp, float* stat, float* ent_out, float* ws,
                  void* stream);
/* out = {#(mask > 0), sum(mask)}: the count-normalisers of cdt.py:358-359,386, to be all-reduced under data
 * parallelism and handed to osrl_cdt_loss as `counts` (with `world` = number of equal-sized ranks). */
int osrl_cdt_mask_counts(const float* mask, int32_t BT, float* out, void* stream);
/* d timestep_emb[time_steps[b,t]] += sum of the R token rows of timestep (b,t) in dseq [B, R*T + prefix, E] (atomic
 * scatter) */
int osrl_cdt_timestep_scatter(const float* dseq, const int64_t* time_steps, int32_t B, int32_t T, int32_t R,
                              int32_t prefix, int32_t E, float* dte, void* stream);
/* Input gradients of the token embeddings (cdt.py:178-213) from dseq [B, R*T + prefix, E], the gradient of the
 * pre-LayerNorm sequence: dstates [B*T, od] = dseq(state tokens) W_state, dactions [B*T, ad] likewise, dreturns /
 * dcosts_to_go [B*T] and depisode_cost [B] = the dot products with the 1-wide return / cost / prefix embeddings
 * (dcosts_to_go is the gradient of the cost embedding's input).  An output pointer may be NULL (not computed); every
 * output element is written by one lane in a fixed order (no atomics).  E <= 1024. */
int osrl_cdt_embed_input_grad(const float* dseq, const float* Ws, const float* Wa, const float* Wr, const float* Wc,
                              const float* Wp, int32_t B, int32_t T, int32_t od, int32_t ad, int32_t E, int32_t use_rew,
                              int32_t use_cost, int32_t prefix, float* dstates, float* dactions, float* dreturns,
                              float* dcosts_to_go, float* depisode_cost, void* stream);
/* torch.nn.utils.clip_grad_norm_ (cdt.py:398-399): out[0] = min(1, clip/(||grad||+1e-6)), out[1] = ||grad|| */
int osrl_clip_grad_scale(const float* grad, int64_t n, float clip, float* partial_ws, int32_t n_parts, float* out,
                         void* stream);
/* Adam step on log_temperature with loss exp(logT)*(entropy - target) (cdt.py:402-407); moments = {m, v} */
int osrl_cdt_temperature_step(float* log_temperature, float* moments, const float* entropy, float target_entropy,
                              float lr, float beta1, float beta2, float eps, const osrl_step_state_t* st, void* stream);

/* ---- BEAR-Lagrangian glue (osrl/algorithms/bearl.py) ----
 * Rows are batch-major: row b*M + j = sample j of batch element b (repeat_interleave, bearl.py:224-226).
 * osrl_bear_mmd: u = mu + exp(clamp(log_std)) * eps from the actor head [B*M, 2*ad] (net.py:176-186);
 *   mmd[b] = mmd_loss_gaussian / mmd_loss_laplacian(raw_vae[b], u[b], sigma) (bearl.py:277-312);
 *   du = d mmd[b] / d u (unscaled); tanh_u = tanh(u); a0[b] = tanh(u[b, 0]) (the critics' action, bearl.py:243-245).
 *   M <= 64, ad <= 16. */
enum { OSRL_MMD_GAUSSIAN = 0, OSRL_MMD_LAPLACIAN = 1 };
int osrl_bear_mmd(const float* raw_vae, const float* head, const float* eps, int32_t rows, int32_t n_samples,
                  int32_t ad, float sigma, int32_t kernel, float* mmd, float* du, float* tanh_u, float* a0,
                  void* stream);
/* out = {mean min(q1,q2), mean min(qc1,qc2), mean mmd} over rows / rows_global: the data-parallel pre-pass (the PID
 * controller and the dual step need GLOBAL means); all-reduce it and pass it as global_means below. */
int osrl_bear_actor_sums(const float* q, int32_t nq1, int32_t nq2, const float* qc, int32_t nc1, int32_t nc2,
                         const float* mmd, int32_t rows, int32_t rows_global, float* out, void* stream);
/* The scalar side of BEARL.actor_loss (bearl.py:246-275): PID multiplier (net.py:376-387, state pid[2]); loss =
 * mean(-q [only once n_train_steps = st->step - 1 >= start_update_policy_step] + exp(log_alpha)*(mmd - thresh)) +
 * mean((qc - qc_thres) * multiplier); dq / dqc = d loss / d (every Q-net output) with torch.min's routing;
 * coef[0] = exp(log_alpha) / rows_global BEFORE the dual step log_alpha += alpha_lr*exp(log_alpha)*mean(mmd - thresh),
 * clamp [-5, 5]; stat[0..5) = actor_loss, mmd_loss, qc_penalty, lagrangian, alpha_value (x stat_share). */
int osrl_bear_actor_loss(const float* q, int32_t nq1, int32_t nq2, const float* qc, int32_t nc1, int32_t nc2,
                         const float* mmd, int32_t rows, float qc_thres, float KP, float KI, float KD,
                         float target_mmd_thresh, float alpha_lr, int64_t start_update_policy_step,
                         int32_t rows_global, const float* global_means, float stat_share,
                         const osrl_step_state_t* st, float* pid, float* log_alpha, float* dq, float* dqc, float* coef,
                         float* stat, void* stream);
/* dhead[B*M, 2*ad] = d loss / d (mu, log_std): du = coef[0]*du_mmd + [sample 0] sum_nets da_nets[n, b] * (1 - tanh_u^2);
 * d mu = du, d log_std = du * eps * std inside the clamp range (net.py:180). */
int osrl_bear_head_bwd(const float* head, const float* eps, const float* tanh_u, const float* du_mmd, const float* coef,
                       const float* da_nets, int32_t n_nets, int32_t rows, int32_t n_samples, int32_t ad, float* dhead,
                       void* stream);

/* ---- COptiDICE glue (osrl/algorithms/coptidice.py) ----
 * nu2 / chi2 = EnsembleQCritic outputs [n_nets, 2*rows] on the stacked rows [obs; next_obs].
 * leaves = float[6] {tau, m, v, lmbda, m, v}: the raw scalar leaves (coptidice.py:96-97) with their Adam moments;
 * work = float[4] {softplus(lmbda), softplus(tau), weighted_c, -} of the current step. */
enum { OSRL_F_CHI2 = 0, OSRL_F_SOFTCHI = 1, OSRL_F_KL = 2 }; /* get_f_div_fn, coptidice.py:15-38 */
/* _optimal_w (coptidice.py:122-131): e = r - lambda' c + gamma (1-d) min nu(s') - min nu(s), w = relu(f'^-1(e/alpha)).
 * use_saved_lambda = 0: lambda' = softplus(leaves[3]) and work[0..1] are (re)written (top of update(), :138);
 * 1: lambda' = work[0] (policy extraction after the lambda step, :211-213).  e may be NULL. */
int osrl_dice_optimal_w(const float* nu2, int32_t n_nu, int32_t rows, const float* rew, const float* cost,
                        const float* done, const float* leaves, float* work, int32_t use_saved_lambda, float alpha,
                        float gamma, int32_t f_type, float* e, float* w, void* stream);
/* coptidice.py:149-185: ell, the softmax over the WHOLE batch, D_kl, weighted_c -> work[2], chi_loss and its gradient
 * dchi [n_chi, 2*rows] (weights are not detached in the reference), Adam step on tau; stat[0..3) = chi_loss, tau_loss,
 * D_kl.  chi2 == NULL (cost_ub_epsilon == 0): weighted_c = mean(w c), zero stats, no update.
 * Data parallel: osrl_dice_chi_ell writes this rank's ell [rows]; the caller all-gathers it into ell_all
 * [rows_global] and passes it with this rank's first row row0: the softmax statistics are then the GLOBAL ones
 * (identical on every rank, written x stat_share because the statistics vector is all-reduced), work[2] is this
 * rank's share of weighted_c (all-reduce it), dchi covers this rank's rows.  ell_all == NULL: one GPU. */
int osrl_dice_chi_ell(const float* chi2, int32_t n_chi, int32_t rows, const float* w, const float* cost,
                      const float* done, const float* is_init, float gamma, float init_state_propotion, float* ell,
                      void* stream);
int osrl_dice_chi_step(const float* chi2, int32_t n_chi, int32_t rows, const float* w, const float* cost,
                       const float* done, const float* is_init, float gamma, float init_state_propotion,
                       float cost_ub_epsilon, float scalar_lr, const osrl_step_state_t* st, float* leaves, float* work,
                       float* ell_ws, float* dchi, const float* ell_all, int32_t rows_global, int32_t row0,
                       float stat_share, float* stat, void* stream);
/* coptidice.py:147,188-201: Df, td_error, nu_loss (this rank's share of the global means: 1/rows_global) and dnu
 * [n_nu, 2*rows]; lmbda_loss and the Adam step on lmbda from the GLOBAL weighted_c in work[2];
 * stat[0..7) = Df, td_error, nu_loss, lmbda_loss, (untouched: actor_loss), tau', lambda' (the last three x stat_share). */
int osrl_dice_nu_step(const float* nu2, int32_t n_nu, int32_t rows, const float* e, const float* w, const float* done,
                      const float* is_init, int32_t f_type, float gamma, float alpha, float init_state_propotion,
                      float qc_thres, float scalar_lr, int32_t rows_global, float stat_share,
                      const osrl_step_state_t* st, float* leaves, const float* work, float* dnu, float* stat,
                      void* stream);
/* out = x + eps * std[col] * scale (coptidice.py:204-205; std is [1, dim]) */
int osrl_dice_perturb(const float* x, const float* eps, const float* std, int32_t rows, int32_t dim, float scale,
                      float* out, void* stream);
/* coptidice.py:207-215: actor_loss = -mean(w * sum Normal(mu, exp(clamp(log_std))).log_prob(act)) (pre-tanh Gaussian,
 * mean over rows_global), dhead [rows, 2*ad] = its gradient w.r.t. (mu, log_std); stat[0] = actor_loss (share). */
int osrl_dice_actor_loss(const float* head, const float* act, const float* w, int32_t rows, int32_t ad,
                         int32_t rows_global, float* dhead, float* stat, void* stream);

/* ---- dataset ingestion on device (osrl/common/dataset.py) ----
 * The flat DSRL arrays (observations, actions, rewards, costs, terminals, timeouts) are uploaded once; these calls
 * produce, in HBM, what the reference computes in host python loops before training.  `ws` is an int32 workspace of
 * osrl_ingest_ws_elems(n) elements; n < 2^31.  Index outputs are exact, fp32 recurrences bit-identical to numpy. */
int64_t osrl_ingest_ws_elems(int64_t n);
/* Episode split at `terminals == 1 || timeouts == 1` (dataset.py:60, :165): ep_end[e] = index of the e-th done
 * flag, ep_start[e] = ep_end[e-1] + 1, ep_len[e]; *n_episodes = number of COMPLETE episodes (transitions after the
 * last done flag belong to none, as in process_sequence_dataset dataset.py:156-175).  ep_* are sized n. */
int osrl_episode_segments(const float* terminals, const float* timeouts, int64_t n, int64_t* ep_end, int64_t* ep_start,
                          int32_t* ep_len, int32_t* n_episodes, int32_t* ws, void* stream);
/* discounted_cumsum (dataset.py:19-27) per episode: out[t] = x[t] + gamma*out[t+1].  reverse: x -> 1 - x first
 * (cost_reverse, dataset.py:161-162; x_out, optional, receives the transformed x).  broadcast_first: every step of
 * the episode gets out[first step] (process_bc_dataset dataset.py:63-70; steps outside episodes are not written). */
int osrl_episode_returns(const float* x, const int64_t* ep_start, const int32_t* ep_len, int32_t n_episodes,
                         float gamma, int32_t reverse, int32_t broadcast_first, float* out, float* x_out, void* stream);
/* compute_cost_sample_prob (dataset.py:439-459): prob[e] = max(T(c_e), 0) / sum, c_e = cost_returns[ep_start[e]],
 * T(c) = a*c + b (OSRL_COST_AFFINE; the reference default 50 - c, train_cdt.py:139 70 - c) or 1/(c + b)
 * (OSRL_COST_RECIPROCAL; train_cdt.py:139 1/(c + 10)); cdf (optional) = its running sum, for
 * osrl_seq_window_gather. */
enum { OSRL_COST_AFFINE = 0, OSRL_COST_RECIPROCAL = 1 };
int osrl_cost_sample_prob(const float* cost_returns, const int64_t* ep_start, int32_t n_episodes, int32_t kind,
                          float a, float b, float* prob, float* cdf, void* stream);
/* compute_start_index_sample_prob (dataset.py:472-494): per trajectory, p[i] ~ (costs (*) gauss_kernel(10,10))[i] + x
 * with x balancing cost / no-cost steps for the target proportion `prob`; p_out / cdf_out are [total rows] laid out
 * like the trajectory tables (either may be NULL); cdf_out feeds osrl_seq_window_gather's start_cdf. */
int osrl_start_index_prob(const float* costs, const int64_t* ep_start, const int32_t* ep_len, int32_t n_episodes,
                          double prob, float* p_out, float* cdf_out, void* stream);
/* process_bc_dataset's selection (dataset.py:108-124) as a stable compaction: idx[0..*n_keep) = kept transition
 * indices in order.  ALL: every one; SAFE: cr <= t0; RISKY: cr >= t0; BOUNDARY: t0 < cr <= t1 (the caller passes
 * the thresholds cost_limit, 2 x cost_limit, (0.5, 1.5) x cost_limit rounded to fp32 as numpy does). */
enum { OSRL_BC_ALL = 0, OSRL_BC_SAFE = 1, OSRL_BC_RISKY = 2, OSRL_BC_BOUNDARY = 3 };
int osrl_bc_select(const float* cost_returns, int64_t n, int32_t mode, float t0, float t1, int64_t* idx,
                   int32_t* n_keep, int32_t* ws, void* stream);
/* dst[j, :width] = src[idx[j], :width]; extra (optional): dst[j, width] = extra[idx[j]] (BC multi-task appends the
 * cost return to the observation, dataset.py:128-130). */
int osrl_gather_rows(const float* src, int32_t width, const int64_t* idx, int64_t n_rows, float* dst, int32_t dst_ld,
                     const float* extra, void* stream);

/* ---- Pareto-frontier augmentation (osrl/common/dataset.py:186-396, :557-630, :47-92) ----
 * The CDT dataset recipe (augmentation / random_augmentation) and process_bc_dataset's "frontier" mode over the
 * tables above, fp64 per trajectory as numpy.  Each `ws` is a workspace of the matching *_ws_elems() 8-byte
 * elements.  Random draws come from Philox keyed by `seed` unless an injected array (any may be NULL) is given: then
 * its values are used in the reference's order of use -- pick_in: the positions random.sample keeps inside every
 * overfull bin ([overfull bins][max_per_bin], dict order); u_rew / u_part / u_cr: the random_sample() doubles that
 * np.random.uniform / np.random.choice consume; noise_c / noise_r: the np.random.normal rows, [augmented rows]. */
/* r0[e] = returns[traj_start[e]], c0[e] = cost_returns[traj_start[e]], widened to fp64 */
int osrl_traj_returns(const float* ret, const float* cret, const int64_t* traj_start, int32_t n_traj, double* r0,
                      double* c0, void* stream);
/* grid_filter (dataset.py:239-272) with the data's own bounds: numpy floor_divide bin keys, bins in dict order
 * (first member), members in index order, > max_per_bin -> max_per_bin drawn, <= min_per_bin -> dropped.
 * filt[0..*count) = kept indices (n sized), fx / fy = x / y at them; *count = -1 when a bin width is 0.
 * n <= 2^20, (xbins+1)(ybins+1) <= 576, max_per_bin <= 32. */
int64_t osrl_grid_filter_ws_elems(int64_t n);
int osrl_grid_filter(const double* x, const double* y, int32_t n, int32_t xbins, int32_t ybins, int32_t max_per_bin,
                     int32_t min_per_bin, const int32_t* pick_in, uint64_t seed, int32_t* filt, double* fx, double* fy,
                     int32_t* count, void* ws, void* stream);
/* oapackage ParetoDoubleLong over (-c, r): flag[i] = 1 iff no point is >= in both and > in one; n <= 2^20 */
int osrl_pareto_mask(const double* c, const double* r, int32_t n, int32_t* flag, void* stream);
/* np.polyfit(x[P], y[P], deg), P = flagged indices in order (flag NULL: all): coef[0..deg] highest power first,
 * pidx[0..*pcount) = P.  pick != 0: process_bc_dataset's rule, deg 0, 1, 2 until r^2 >= 0.9 (*deg_out = the one
 * kept).  stats[5] = {r2 deg 0, 1, 2 (NaN if not tried), max y, min y over all n}.  deg <= 7. */
int64_t osrl_polyfit_ws_elems(int64_t n, int32_t deg);
int osrl_polyfit(const double* x, const double* y, const int32_t* flag, int32_t n, int32_t deg, int32_t pick,
                 double* coef, int32_t* deg_out, int32_t* pidx, int32_t* pcount, double* stats, void* ws, void* stream);
/* augmentation()'s targets + get_nearest_point (dataset.py:186-236, :350-366) over the F filtered points:
 * tc = linspace(min fx, max fx, S), tr = U[pf(tc) + min_reward, max_reward]; nearest[0..S) = get_nearest_point's
 * index list (unique nearest indices in first-occurrence order, each followed by its drawn partners).  F <= 8000. */
int64_t osrl_augment_targets_ws_elems(int64_t F, int64_t S);
int osrl_augment_targets(const double* coef, const int32_t* deg, const double* fx, const double* fy, int32_t F,
                         int32_t S, double min_reward, double max_reward, double max_rew_decrease, double beta,
                         const double* u_rew, const double* u_part, uint64_t seed, double* tc, double* tr,
                         int32_t* nearest, void* ws, void* stream);
/* random_augmentation's targets (dataset.py:586-615): (tc, tr) uniform in [aug_cmin, aug_cmax] x [aug_rmin,
 * aug_rmax]; nearest[k] = masked argmin of hypot over c0 <= max(tc - cgap, min c0 + 1). */
int osrl_random_aug_targets(const double* c0, const double* r0, int32_t n, int32_t S, double aug_cmin, double aug_cmax,
                            double aug_rmin, double aug_rmax, double cgap, const double* u_cr, uint64_t seed,
                            double* tc, double* tr, int32_t* nearest, void* stream);
/* combined trajectory table: the n_traj originals, then one copy of src[k] = map[nearest[k]] (map NULL: nearest[k])
 * per sample, rows appended after n_rows; new_* are [n_traj + S]; *total = rows of the combined tables. */
int osrl_augment_layout(const int32_t* nearest, const int32_t* map, int32_t S, const int64_t* traj_start,
                        const int32_t* traj_len, int32_t n_traj, int64_t n_rows, int64_t* new_start, int32_t* new_len,
                        int32_t* src, int64_t* total, void* stream);
/* the augmented rows of the combined tables (the original rows are the caller's copy): observations, actions,
 * rewards, costs bit for bit; returns / cost_returns = fp32(fp64(x) + ((target - fp64(x[0])) [+ noise])), noise
 * (random_augmentation) N(0, cstd) / N(0, rstd) per row. */
int osrl_augment_gather(const float* obs, const float* act, const float* rew, const float* cost, const float* ret,
                        const float* cret, int32_t od, int32_t ad, const int64_t* traj_start, const int32_t* src,
                        int32_t S, const int64_t* new_start, const int32_t* new_len, int32_t n_traj, const double* tc,
                        const double* tr, int32_t noise, double cstd, double rstd, const double* noise_c,
                        const double* noise_r, uint64_t seed, float* o_obs, float* o_act, float* o_rew, float* o_cost,
                        float* o_ret, float* o_cret, void* stream);
/* process_bc_dataset "frontier" (dataset.py:91-93, :111): keep transition i iff |rr_i - pf(cr_i)| <= (rmax-rmin)/5
 * (coef / deg / stats from osrl_polyfit with pick); mask [n] floats of scratch; then osrl_bc_select's compaction. */
int osrl_bc_frontier_select(const float* cost_returns, const float* rew_returns, int64_t n, const double* coef,
                            const int32_t* deg, const double* stats, float* mask, int64_t* idx, int32_t* n_keep,
                            int32_t* ws, void* stream);
/* compute_sample_prob (dataset.py:399-436, SequenceDataset(pf_sample=True)): w_i = 1 / (dist_i + beta), dist_i the
 * distance of (c, r) = (cost_returns, returns)[traj_start[i]] to the frontier p (coef / deg from osrl_polyfit) as the
 * reference's BFGS solve arrives at it: with f(x) = (x-c)^2 + (p(x)-r)^2 and g = f'/2, x* = c if g(c) == 0, else the
 * first root of g with a sign change downhill from c (below c if g(c) > 0, above if g(c) < 0); x = max(0, x*),
 * dist = sqrt(f(x)).  The roots are isolated through the derivative chain and bisected to fp64 resolution
 * (csrc/pf_dist.h); fp64 throughout, one thread per trajectory.  prob = w / sum w and cdf (optional) = its inclusive
 * running sum, fp32, summed in fp64 in a fixed order (the same bits on every run).  dist (optional): [n_traj] fp64.
 * ws: [n_traj] doubles.  n_traj <= 2^20, deg <= 7, beta > 0. */
int osrl_pf_sample_prob(const float* returns, const float* cost_returns, const int64_t* traj_start, int32_t n_traj,
                        const double* coef, const int32_t* deg, double beta, float* prob, float* cdf, double* dist,
                        double* ws, void* stream);
/* prob[i] = max(weights[i], 0) / sum, cdf (optional) = inclusive running sum / sum, from any per-trajectory fp64
 * weights on device (SequenceStore.set_sample_prob; a python cost_transform applied on the host); n <= 2^20. */
int osrl_weights_sample_prob(const double* weights, int32_t n, float* prob, float* cdf, void* stream);

/* ---- batched on-device evaluation ----
 * The reference's Trainer.rollout (cpq.py:330-347, bcql.py:323-340, bc.py:125-145) steps ONE gym env per policy
 * call and crosses host<->device every env step.  No gym env exists in either container, so the build owns a
 * synthetic safe environment (osrl_amd/common/synthetic_env.py: s' = A s + Bm clip(a), reward = 1 - 0.1|s'-goal|^2,
 * cost = 1[s'.w > threshold]); this is its vectorised device step: one row per episode.
 *   state[E, state_dim]  in/out;  obs[E, obs_ld] receives s' in its first state_dim columns (the policy's input
 *   buffer; extra columns, e.g. BC multi-task's cost_limit, are left alone);
 *   acc[E,4] = {return, cost*cost_scale, length, done}: accumulated here, done latches at episode_len and freezes
 *   the episode (state, obs and totals stop changing). */
typedef struct {
  const float* At;   /* A transposed:  At[j*state_dim + i] = A[i][j]   (coalesced per-output reads) */
  const float* Bt;   /* Bm transposed: Bt[k*state_dim + i] = Bm[i][k] */
  const float* w;    /* [state_dim] cost half-space normal */
  const float* goal; /* [state_dim] */
  int32_t state_dim, action_dim, episode_len, pad_;
  float max_action, cost_threshold, cost_scale, pad2_;
} osrl_env_t;
int osrl_env_step(const osrl_env_t* env, const float* act, float* state, float* obs, int32_t obs_ld, float* acc,
                  float* step_out /* optional [E,2]: this step's (reward, raw cost) */, int32_t episodes, void* stream);

/* osrl_env_step with exploration noise, recording what it does: one launch perturbs the policy's action, steps the
 * environment with osrl_env_step's arithmetic (bit for bit), writes the transition into DSRL-layout tables and keeps the
 * discounted sums.  Episode ep at its own step t = acc[ep][2] (t < episode_len, done latch clear; otherwise the launch
 * writes nothing for it):
 *   a = clip(act[ep] + sigma[ep] * eps, +-max_action); sigma[ep] == 0 gives exactly clip(act[ep]) (eps is not read);
 *   eps = eps_in[(t * episodes + ep) * action_dim + k] when eps_in is given, else word (k & 3) -> N(0,1) (the map of
 *         osrl_randn_fill) of Philox4x32-10(counter {episode_base + ep, t, k >> 2, stream_id}, key *seed): a function of
 *         (seed, episode id, step, column) alone;
 *   row ep * episode_len + t of the tables: observations = s, actions = a, next_observations = s', rewards, costs (raw
 *         0 / 1), terminals = 0, timeouts = (t + 1 >= episode_len);
 *   disc[ep] = {sum gamma^t r, sum gamma^t cost * cost_scale, gamma^t (start: 1), unused}.
 * seed, gamma and sigma are read from device memory: a captured launch follows their current values. */
typedef struct {
  float* observations;      /* [episodes * episode_len, state_dim] */
  float* actions;           /* [episodes * episode_len, action_dim] */
  float* next_observations; /* [episodes * episode_len, state_dim] */
  float* rewards;           /* [episodes * episode_len] */
  float* costs;
  float* terminals;
  float* timeouts;
  float* disc;              /* [episodes, 4] */
  const float* sigma;       /* [episodes] */
  const float* gamma;       /* [1] */
  const uint64_t* seed;     /* [1] */
  const float* eps_in;      /* [episode_len, episodes, action_dim] or NULL */
  uint32_t episode_base;
  uint32_t stream_id;
} osrl_collect_t;
int osrl_env_collect(const osrl_env_t* env, const osrl_collect_t* rec, const float* act, float* state, float* obs,
                     int32_t obs_ld, float* acc, int32_t episodes, void* stream);

/* CDTTrainer.rollout (cdt.py:436-518) with E episodes as batch rows.  The reference keeps the whole history and
 * slices its last seq_len steps per env step; here the CDT engine's [E, seq_len] batch buffers are the window
 * itself: left-aligned and growing (mask = 1 on the filled prefix) until full, then sliding by one per env step.
 * cursor: device int32 = env steps taken so far (identical for all episodes).
 *   pick: act[e] = clamp(head[e, last filled position, :action_dim], +-max_action)     (cdt.py:489-493)
 *   push (after osrl_env_step): actions[last] = act; append (obs', returns - reward, costs_to_go - cost*cost_scale
 *         [1 - cost under cost_reverse], time step + 1, zero dummy action) (cdt.py:496-508); ++cursor.  The pick at
 *         cursor == episode_len reads the last window; callers stop there. */
int osrl_cdt_rollout_pick(const float* head, int32_t head_width, int32_t action_dim, int32_t episodes,
                          int32_t seq_len, const int32_t* cursor, float max_action, float* act, void* stream);
int osrl_cdt_rollout_push(float* states, float* actions, float* returns, float* costs_to_go, int64_t* time_steps,
                          float* mask, int32_t episodes, int32_t seq_len, int32_t state_dim, int32_t action_dim,
                          const float* act, const float* obs, int32_t obs_ld, const float* step_out, float cost_scale,
                          int32_t cost_reverse, int32_t* cursor, int32_t episode_len /* no-op once cursor reaches it */,
                          void* stream);

/* The CDT rollout step that records: pick, osrl_env_step, push and the cursor of the rollout above, plus what
 * osrl_env_collect adds to a step, as ONE launch after the transformer forward (one workgroup per episode, no shared
 * cursor).  Episode ep at its own step t = acc[ep][2] (t < episode_len, done latch clear; otherwise the launch writes
 * nothing for it), its window holding n = min(t + 1, seq_len) filled positions:
 *   mu = head[(ep * seq_len + n - 1) * head_width + k];  s = sample ? exp(head[... + action_dim + k]) (rows are
 *         [mu | log_std], no log-std bounds, head_width >= 2 * action_dim) : rec->sigma[ep];
 *   a = clip(mu + s * eps, +-max_action), eps as osrl_env_collect documents it; s == 0 gives exactly clip(mu) and eps
 *         is not read;
 *   the environment step, the table row ep * episode_len + t, acc (cost sum * env->cost_scale) and rec->disc:
 *         osrl_env_collect's arithmetic, bit for bit;
 *   the window: actions[n - 1] = a, then (sliding by one when n == seq_len) append s', returns - reward, costs_to_go -
 *         cost * win->cost_scale [1 - cost under cost_reverse], time step t + 1, a zero dummy action, mask = 1 --
 *         osrl_cdt_rollout_push's arithmetic.
 * With sigma == 0 and sample == 0 the episode is osrl_cdt_rollout_pick / osrl_env_step / osrl_cdt_rollout_push's, bit
 * for bit.  seq_len <= 1024. */
typedef struct {
  float* states;        /* [episodes, seq_len, state_dim] */
  float* actions;       /* [episodes, seq_len, action_dim] */
  float* returns;       /* [episodes, seq_len] */
  float* costs_to_go;   /* [episodes, seq_len] */
  int64_t* time_steps;  /* [episodes, seq_len] */
  float* mask;          /* [episodes, seq_len] */
  const float* head;    /* [episodes * seq_len, head_width] */
  int32_t seq_len, head_width;
  int32_t sample;       /* 0: s = rec->sigma[ep];  1: s = exp(log_std) of the head row */
  int32_t cost_reverse;
  float cost_scale;     /* of the costs-to-go (acc and disc carry env->cost_scale) */
  float pad_;
} osrl_cdt_window_t;
int osrl_cdt_collect(const osrl_env_t* env, const osrl_collect_t* rec, const osrl_cdt_window_t* win, float* state,
                     float* acc, int32_t episodes, void* stream);

/* library identity */
/* ---- B = 1 .. OSRL_POLICY_MAX_ROWS act() latency path (act.hip) -----------------------------------------------
 * Replaces one `model.act(obs)` of the reference's episode loop (XTrainer.rollout, cpq.py:330-347): H2D copy of the
 * observation + 3-6 aten kernels + two D2H syncs (cpq.py:240-252, bcql.py:236-243, bc.py:66-76) become ONE launch:
 * the observation rows are read from a pinned host buffer mapped into the device, the whole policy (1-2 chained MLPs
 * as GEMVs over the packed forward weights + the distribution head) runs in one workgroup, action / log-prob land
 * in pinned memory and the host spins on a sequence number.  THE ONE EXCEPTION to this header's conventions: a policy
 * handle owns a small pinned host allocation (osrl_policy_create / _destroy) and osrl_policy_act RETURNS AFTER the
 * kernel has published its results (it is the synchronous call the episode loop needs).  Wf / b are DEVICE pointers. */
#define OSRL_POLICY_MAX_ROWS 4
enum { OSRL_POLICY_MLP = 0, OSRL_POLICY_GAUSS = 1, OSRL_POLICY_BCQ = 2 };
typedef struct {
  int32_t n_layers;
  int32_t dims[OSRL_MAX_LAYERS + 1];
  int32_t acts[OSRL_MAX_LAYERS];
  float out_scale;                  /* net output = out_scale * act(z) */
  const float* Wf[OSRL_MAX_LAYERS]; /* PACKED forward weights PF[k/4][n][k%4] (osrl_pack_weights / the fused optimizer
                                     * step keep them in step with the canonical parameters) */
  const float* b[OSRL_MAX_LAYERS];  /* canonical bias [dims[l+1]] */
} osrl_gemv_net_t;
typedef struct {
  int32_t kind;       /* MLP:   a = net0(obs)                               (BC, MLPActor net.py:65-85)
                       * GAUSS: (mu | log_std) = net0(obs); a = max_action * tanh(mu + exp(clamp(ls)) * eps), logp
                       *                                                    (SquashedGaussianMLPActor net.py:152-205)
                       * BCQ:   a0 = net0([obs, clamp(z, +-0.5)]) (VAE.decode net.py:331-339), t = net1([obs, a0]),
                       *        a = clamp(a0 + phi * max_action * t, +-max_action)       (net.py:33-62, bcql.py:236-243) */
  int32_t obs_dim, act_dim, latent_dim;
  float max_action, phi;
  osrl_gemv_net_t net[2];
} osrl_policy_t;
int osrl_policy_create(const osrl_policy_t* desc, void** handle);
/* HOST pointers into the handle's pinned block: obs [MAX_ROWS, obs_dim] (caller writes), noise [MAX_ROWS, act_dim |
 * latent_dim] (caller writes when host_noise = 1), act [MAX_ROWS, act_dim] and logp [MAX_ROWS] (kernel writes). */
int osrl_policy_io(void* handle, float** obs, float** noise, float** act, float** logp);
/* rows <= OSRL_POLICY_MAX_ROWS.  deterministic: eps = 0 (GAUSS).  host_noise: read eps / z from the noise block
 * instead of drawing it in the kernel (Philox keyed by `seed` and the handle's call counter). */
int osrl_policy_act(void* handle, int32_t rows, int32_t deterministic, int32_t host_noise, uint64_t seed, void* stream);
int osrl_policy_destroy(void* handle);

/* ---- lockstep act() path of the same policies (act_vec.hip): n_env episodes on as many host environments, ONE call per
 * environment step for all of them.  Same descriptor, kinds and limits as osrl_policy_create (layers up to
 * OSRL_MAX_WIDTH, OSRL_MAX_LAYERS); falls under the policy-handle exception above.  The slots are padded to 16-row
 * tiles and every layer runs on fp32 MFMA, one workgroup per tile; no arithmetic crosses rows and a dot product's
 * k-order is fixed by the layer shape, so a slot's action does not depend on n_env, on the slot or on its neighbours.
 * 1 <= n_env <= OSRL_POLICY_MAX_ENVS, else -1. */
#define OSRL_POLICY_MAX_ENVS 64
int osrl_policy_create_n(const osrl_policy_t* desc, int32_t n_env, void** handle);
/* HOST pointers into ONE pinned, device-mapped block: obs [n_env, obs_dim], noise [n_env, act_dim | latent_dim] (read
 * when host_noise = 1), active [n_env] (0: the slot idles) and meta [n_env, 2] = (episode id, step) are the caller's
 * to write; act [n_env, act_dim] and logp [n_env] are written by the kernel, for active slots only. */
int osrl_policy_io_n(void* handle, float** obs, float** noise, float** act, float** logp, int32_t** active,
                     int32_t** meta);
/* one environment step of every active slot; returns after all actions have been published.  deterministic / host_noise
 * as osrl_policy_act; noise drawn on the device is Philox keyed by (seed, meta[e][0], meta[e][1], element) only. */
int osrl_policy_act_n(void* handle, int32_t deterministic, int32_t host_noise, uint64_t seed, void* stream);
/* The same call with the EXPLORATION TAIL of the recording collectors on the action of every active slot e (all three
 * kinds; a_pi is the action osrl_policy_act_n publishes -- for GAUSS the scaled, post-tanh one):
 *   a = clip(a_pi + sigma[e] * eps, +-max_action)      (v = fmaf(sigma, eps, v), then the clip: osrl_env_collect's)
 * sigma[e] == 0 publishes exactly a_pi's bits, and eps is not read.  eps is row e of the pinned eps [n_env, act_dim] when
 * host_eps = 1 (injected noise: tests, replays), otherwise the draw osrl_env_collect documents:
 *   word (k & 3) of philox4x32_10(counter = {meta[e][0] = episode id, meta[e][1] = step, k >> 2, stream 13},
 *   key = explore_seed) through the library's word -> N(0,1) map,
 * so a run on host environments records the noise the device collector draws for the same (seed, episode, step, column).
 * This stream is apart from the one `seed` keys (GAUSS's own eps, BCQ's z: untouched).  sigma and eps are the caller's to
 * write (HOST pointers into the handle's pinned block, from _explore_io_n); osrl_policy_act_n reads neither. */
int osrl_policy_explore_io_n(void* handle, float** sigma, float** eps);
int osrl_policy_act_explore_n(void* handle, int32_t deterministic, int32_t host_noise, uint64_t seed,
                              uint64_t explore_seed, int32_t host_eps, void* stream);
int osrl_policy_destroy_n(void* handle);

/* ---- CDT act latency path (cdt_act.hip) ----------------------------------------------------------------------
 * CDTTrainer.rollout (cdt.py:436-518) on a host environment: one action per env step from the window of the last
 * seq_len timesteps.  Falls under the policy-handle exception above: a handle owns a pinned, device-mapped I/O block
 * (observation, taken action, returned action, reward / cost, sequence number) plus the device-resident window and
 * every token's cached hidden state, and _reset / _step RETURN AFTER the action has been published.  Per env step only
 * the work that changed runs: the new tokens while the window grows; from layer-0 attention on
 * while it slides (layer-0 q / k / v stay cached); the cost-prefix token once per episode.
 * Every weight pointer is a DEVICE pointer into the model's flat group: w_* / head_w = PACKED forward weights
 * PF[k/4][n][k%4] (kept current by the fused optimizer step and repack()), the rest canonical row-major tensors.
 * Domain: repeat * seq_len + cost_prefix <= 256 tokens, embedding_dim <= 512, head_dim <= 128, head_layers <= 4,
 * head input / output widths <= 1024; outside it _create returns -1. */
typedef struct {
  const float *ln1_g, *ln1_b, *w_qkv, *b_qkv, *w_o, *b_o, *ln2_g, *ln2_b, *w_1, *b_1, *w_2, *b_2;
} osrl_cdt_layer_t;
typedef struct {
  int32_t state_dim, action_dim, seq_len, embedding_dim, num_layers, num_heads;
  int32_t use_rew, use_cost, cost_prefix, cost_transform; /* cost_transform: the cost token embeds 50 - ctg */
  int32_t add_cost_feat, mul_cost_feat, cat_cost_feat;    /* effective flags (each implies use_cost) */
  int32_t head_layers;    /* Linear layers of the action head (GELU between them) */
  int32_t head_out_width; /* rows of the last head weight: action_dim, or 2 * action_dim for (mu | log_std) */
  int32_t te_rows;        /* rows of the timestep embedding table */
  float max_action;
  int32_t pad_;
  const float* te; /* timestep embedding [te_rows, E]; NULL = time_emb off */
  const float *state_w, *state_b, *action_w, *action_b, *return_w, *return_b, *cost_w, *cost_b, *prefix_w, *prefix_b;
  const float *emb_g, *emb_b, *out_g, *out_b;
  const float* head_w[OSRL_MAX_LAYERS];
  const float* head_b[OSRL_MAX_LAYERS];
} osrl_cdt_policy_t;
/* layers: [num_layers] (copied) */
int osrl_cdt_policy_create(const osrl_cdt_policy_t* desc, const osrl_cdt_layer_t* layers, void** handle);
/* HOST pointers into the pinned block: obs [state_dim] and act_in [action_dim] (caller writes), act_out [action_dim] */
int osrl_cdt_policy_io(void* handle, float** obs, float** act_in, float** act_out);
/* starts an episode at timestep 0 with the observation in obs; the prefix token embeds target_cost */
int osrl_cdt_policy_reset(void* handle, float target_return, float target_cost, void* stream);
/* the previous step's action (act_in when host_action = 1, else the one returned), then obs / reward / cost of the new
 * timestep: returns[t+1] = returns[t] - reward, costs[t+1] = costs[t] - cost (fp32).  -1 past the timestep table. */
int osrl_cdt_policy_step(void* handle, float reward, float cost, int32_t host_action, void* stream);
/* the current window, oldest timestep first: states [n, state_dim], actions [n, action_dim], returns / costs [n],
 * time_steps [n]; n = min(t + 1, seq_len) (0 before the first reset).  Synchronises the stream. */
int osrl_cdt_policy_window(void* handle, float* states, float* actions, float* returns, float* costs,
                           int64_t* time_steps, int32_t* n, void* stream);
int osrl_cdt_policy_destroy(void* handle);
/* N episodes per handle, advanced in LOCKSTEP: every episode is at the same timestep, so one _reset_n / _step_n call runs
 * the same 2 + 5 * layers launches as the one-episode calls, over the rows of all N episodes (a projection's 16-row
 * tiles fill up with rows of several episodes), and returns after all N actions have been published.  An episode's
 * results do not depend on N or on its slot.  A slot whose episode has ended keeps running on whatever its rows of the
 * pinned block hold; the caller ignores its action.  The HANDLE owns the pinned block; the caller writes obs [N,
 * state_dim], act_in [N, action_dim] and scalars [N, 4] = (reward, cost, target_return, target_cost) per episode
 * between calls and reads act_out [N, action_dim] after a call; the pointers die with _destroy.
 * 1 <= n_env <= OSRL_CDT_POLICY_MAX_ENVS, else -1.  _create is _create_n with n_env = 1; _reset / _step serve handles
 * of one episode only (-1 otherwise); _io, _window (episode 0) and _destroy serve both. */
#define OSRL_CDT_POLICY_MAX_ENVS 64
int osrl_cdt_policy_create_n(const osrl_cdt_policy_t* desc, const osrl_cdt_layer_t* layers, int32_t n_env,
                             void** handle);
int osrl_cdt_policy_io_n(void* handle, float** obs, float** act_in, float** act_out, float** scalars);
/* starts N episodes at timestep 0: observations from obs, targets from scalars[e][2..3] */
int osrl_cdt_policy_reset_n(void* handle, void* stream);
/* as _step for every episode: reward and cost from scalars[e][0..1] (scalars[e][2..3] must keep the targets) */
int osrl_cdt_policy_step_n(void* handle, int32_t host_action, void* stream);
/* as _window, of episode env (0 <= env < n_env, else -1), at that episode's own timestep */
int osrl_cdt_policy_window_n(void* handle, int32_t env, float* states, float* actions, float* returns, float* costs,
                             int64_t* time_steps, int32_t* n, void* stream);
/* Slots at INDEPENDENT timesteps: one call in which every episode idles (mode[e] = 0), steps (1) or restarts (2), still
 * 2 + 5 * layers launches.  A restarting episode begins at timestep 0 from obs[e] and scalars[e][2..3] (the prefix token
 * is embedded again); a stepping one reads scalars[e][0..1] and, with host_action = 1, act_in[e]; an idle one runs no
 * rows, keeps its window and timestep and can be continued by a later call, and its row of act_out is not written.
 * Every episode contributes the rows of its own phase (the host derives them per call from the episodes' timesteps), so
 * an episode's results are the bits the one-episode handle returns for the same inputs, whatever the others do.
 * _reset_n is this call with every mode 2, _step_n with every mode 1.  Returns -1, and changes nothing, if a stepping
 * episode was never started or is past the timestep table, or on a mode outside 0 .. 2; 0 at once if all idle. */
int osrl_cdt_policy_step_slots(void* handle, const int32_t* mode, int32_t host_action, void* stream);
/* t [n_env]: the timestep of each episode's newest window entry, -1 = never started */
int osrl_cdt_policy_timesteps(void* handle, int32_t* t);
/* _step_slots with the EXPLORATION TAIL of osrl_cdt_collect on the action of every episode e that runs:
 *   a = clip(mu + s * eps, +-max_action);  s = sample ? exp(log_std) of the head row (no log-std bounds; needs
 *         head_out_width >= 2 * action_dim, else -1) : sigma[e];  s == 0 gives clip(mu) exactly and eps is not read;
 *   eps = row e of the pinned eps [n_env, action_dim] when host_eps = 1, otherwise word (k & 3) of philox4x32_10(counter
 *         = {episode_id[e], the episode's own timestep, k >> 2, stream 13}, key = explore_seed) through the library's word
 *         -> N(0,1) map: osrl_env_collect's draw.
 * mu is the evaluating call's bits (the log_std columns are computed in a pass of their own with the mean's k-split), and
 * the action TAKEN is what the window records at the next step (unless host_action = 1 overrides it).  With sample = 1
 * the head row (mu | log_std) of every episode that ran is written to head [n_env, 2 * action_dim], for the caller's
 * behaviour log-probabilities.  sigma [n_env], eps, episode_id [n_env] and head are HOST pointers into the handle's pinned
 * block (_explore_io); the calls without the tail read none of them. */
int osrl_cdt_policy_explore_io(void* handle, float** sigma, float** eps, int32_t** episode_id, float** head);
int osrl_cdt_policy_step_slots_explore(void* handle, const int32_t* mode, int32_t host_action, int32_t sample,
                                       uint64_t explore_seed, int32_t host_eps, void* stream);

/* ---- data-parallel exchanges through IPC-mapped device buffers (ipc.hip, round 6; nothing to mirror in the reference: it
 * has no distributed code).  What the ranks of a data-parallel step exchange (flat
 * gradients per optimizer phase, CPQ's KL values, statistics) is latency-bound; a collective-library launch costs 16-19 us
 * even on one rank.  Here every rank owns a published buffer (2 halves of half_floats) and a 64-byte control block in ITS
 * device memory (osrl_ipc_alloc), hands the two handles to its peers by any means (the engines use torch.distributed's
 * object all-gather, once) and maps theirs (osrl_ipc_open).  An exchange is ONE asynchronous, hipGraph-capturable kernel
 * launch per rank: publish -> flag -> wait for every rank's flag -> sum in RANK ORDER (replicas stay bit-identical) or
 * gather.  Every rank must issue the same sequence of exchanges on ONE stream; a peer that never arrives makes the launch
 * give up after ~2 s and set the error word (osrl_ipc_status), it does not hang the device. */
#define OSRL_IPC_MAX_WORLD 8
#define OSRL_IPC_MAX_SEG 8
#define OSRL_IPC_HANDLE_BYTES 64
typedef struct {
  int32_t world, rank;
  float* pub[OSRL_IPC_MAX_WORLD];    /* published buffers, [rank] = this process's own allocation, the others mapped */
  uint32_t* ctl[OSRL_IPC_MAX_WORLD]; /* control blocks (>= 64 bytes, zeroed): flag | arrivals | error | exchanges done */
  int64_t half_floats;               /* floats per published half (a message must fit; multiple of 4) */
} osrl_ipc_t;
/* hipMalloc + zero + hipIpcGetMemHandle / hipIpcOpenMemHandle / Close / hipFree (setup time, synchronous). */
int osrl_ipc_alloc(int64_t bytes, void** dev_ptr, void* handle64);
int osrl_ipc_open(const void* handle64, void** dev_ptr);
int osrl_ipc_close(void* mapped_ptr);
int osrl_ipc_free(void* dev_ptr);
/* bufs[i][0 .. lens[i]) += the same ranges of every other rank (in place, n_bufs <= OSRL_IPC_MAX_SEG, together <=
 * half_floats: OSRL_E_UNSUPPORTED otherwise) -- dist.all_reduce(SUM) of several tensors as one launch. */
int osrl_ipc_all_reduce(const osrl_ipc_t* x, float* const* bufs, const int64_t* lens, int32_t n_bufs, void* stream);
/* The same where bufs[i] is slab 0 of n_slabs[i] split-K gradient slabs slab_strides[i] floats apart (what the dW kernels
 * leave): the rank's own slab sum -- slab order, the bits of osrl_reduce_slabs -- is formed while publishing, and slab 0
 * receives the sum over slabs AND ranks: osrl_reduce_slabs + osrl_ipc_all_reduce in one launch. */
int osrl_ipc_all_reduce_slabs(const osrl_ipc_t* x, float* const* bufs, const int64_t* lens, const int32_t* n_slabs,
                              const int64_t* slab_strides, int32_t n_bufs, void* stream);
/* dst[r * n + i] = rank r's src[i] -- dist.all_gather_into_tensor. */
int osrl_ipc_all_gather(const osrl_ipc_t* x, const float* src, int64_t n, float* dst, void* stream);
/* words4 = this rank's control words (flag, arrivals, error: 0 = fine, 1 + r = rank r never arrived, exchanges done).
 * Synchronous copy: for the points where the host synchronises anyway. */
int osrl_ipc_status(const osrl_ipc_t* x, uint32_t* words4);

/* ---- learned-dynamics vector environment (model_env.hip) -----------------------------------------------------------
 * An ensemble of n_models ReLU MLPs [state_dim + action_dim, hidden.., state_dim + 2] fitted on logged transitions
 * (osrl_amd/algorithms/dynamics.py), stepped as a vector environment with osrl_env_step's interface and bookkeeping:
 * one launch per environment step, one workgroup per 16-episode tile, the whole ensemble with its activations in LDS
 * (act_vec.hip's layer scheme over the packed forward weights, which the fused optimizer step keeps current: the
 * environment follows training in place).  Every layer dimension <= 512, state_dim <= 256.
 * Per live episode e (acc[e][3] == 0; a finished one keeps state, obs and totals):
 *   x = [(s - mu_s) / sd_s, clip(a, +-max_action)];  y_m = net_m(x), m = 0 .. n_models - 1;
 *   ybar = (y_0 + y_1 + ..., in that order) * (1 / n_models);
 *   d = max_m sqrt(sum_{k < state_dim} (y_m[k] - ybar[k])^2 / state_dim)      (the members' disagreement, normalised units)
 *   yh = ybar (MEAN) | y_member (MEMBER) | y_j (RANDOM: j = member_in[e] when member_in is given, else word x of
 *        Philox4x32-10(counter {episode_base + e, the episode's step acc[e][2], 0, 14}, key *seed) mod n_models);
 *        every mode evaluates every member, member k's output has the same bits in each;
 *   s' = s + (mu_d + sd_d * yh[:state_dim]), clamped to [s_lo, s_hi] when both are given;
 *   r = mu_r + sd_r * yh[state_dim], minus reward_penalty * d when reward_penalty != 0;
 *   cost = yh[state_dim + 1] > 0.5 ? 1 : 0;
 *   acc / step_out / state / obs: osrl_env_step's;  unc[e] = {max over steps of d, sum over steps of d}.
 * An episode's trajectory is the same bits whatever `episodes` is, whichever tile row it sits in and whatever its
 * neighbours do (no split-K, no arithmetic across rows). */
enum { OSRL_MODEL_ENV_MEAN = 0, OSRL_MODEL_ENV_MEMBER = 1, OSRL_MODEL_ENV_RANDOM = 2 };
#define OSRL_MODEL_ENV_MAX_WIDTH 512
#define OSRL_MODEL_ENV_MAX_STATE 256
typedef struct {
  osrl_gemv_net_t net[OSRL_MAX_NETS]; /* out_scale 1, identity output */
  const float* mu_s;  /* [state_dim] */
  const float* sd_s;  /* [state_dim] */
  const float* mu_d;  /* [state_dim] */
  const float* sd_d;  /* [state_dim] */
  const float* mu_r;  /* [1] */
  const float* sd_r;  /* [1] */
  const float* s_lo;  /* [state_dim] or NULL (with s_hi): no clamp */
  const float* s_hi;
  const uint64_t* seed;     /* [1], read in RANDOM mode without member_in */
  const int32_t* member_in; /* [episodes] or NULL */
  int32_t n_models, state_dim, action_dim, episode_len;
  int32_t mode, member;
  uint32_t episode_base;
  int32_t pad_;
  float max_action, cost_scale, reward_penalty, pad2_;
} osrl_model_env_t;
int osrl_model_env_step(const osrl_model_env_t* env, const float* act, float* state, float* obs, int32_t obs_ld,
                        float* acc, float* unc /* [E,2] */, float* step_out /* optional [E,2] */, int32_t episodes,
                        void* stream);
/* osrl_model_env_step with exploration noise, recording what it does (engine/collect.py ModelCollector): the same launch
 * shape and the same body behind a compile-time flag, plus what osrl_env_collect adds to osrl_env_step.  Episode e at its
 * own step t = acc[e][2] (read once per launch; 0 <= t < env->episode_len and the done latch clear, otherwise the launch
 * stores nothing for it -- so no write leaves the tables, whose rows are episodes * env->episode_len):
 *   a = clip(fmaf(sigma[e], eps, act[e]), +-max_action) while the input tile is staged; sigma[e] == 0: eps is not read and
 *       the step is osrl_model_env_step's bit for bit;  eps as osrl_env_collect documents it (eps_in or Philox on
 *       rec->stream_id, keyed by (seed, episode_base + e, t, column));
 *   row e * episode_len + t: observations = s, actions = a, next_observations = s' (after the clamp), rewards = r (after
 *       reward_penalty: what acc[e][0] sums), costs (raw 0 / 1), terminals = 0, timeouts = (t + 1 >= episode_len);
 *   rec->disc as osrl_env_collect keeps it;  row_unc (optional [episodes * episode_len]) receives the row's d. */
int osrl_model_env_collect(const osrl_model_env_t* env, const osrl_collect_t* rec, const float* act, float* state,
                           float* obs, int32_t obs_ld, float* acc, float* unc,
                           float* row_unc /* optional [E * episode_len] */, int32_t episodes, void* stream);
/* The same two launches on an ensemble of diagonal Gaussians (algorithms/dynamics.py, probabilistic=True): member m's
 * output row is (od + 1 means | raw cost | od + 1 raw log-variances), 2 od + 3 <= OSRL_MODEL_ENV_MAX_WIDTH columns; the
 * first od + 2 are read exactly as osrl_model_env_step reads them.  With P = od + 1 and, for k < P,
 *   lv_m[k] = lo + softplus((hi - softplus(hi - raw_m[k])) - lo),  raw_m[k] = y_m[od + 2 + k],  sg_m[k] = exp(0.5 lv_m[k]):
 *   d = osrl_model_env_step's disagreement over the MEANS, the same expression;
 *   a = max_m sqrt(sum_{k < od} sg_m[k]^2 / od)               (MOPO's largest predicted standard deviation)
 *   u = d (uncertainty == OSRL_MODEL_ENV_UNC_DISAGREEMENT) | a (OSRL_MODEL_ENV_UNC_MAX_STD): u takes d's place in the
 *       reward penalty, in unc[e] and in row_unc;
 *   sample != 0:  v[k] = sg_f[k]^2 of the followed member f (MEMBER, RANDOM) | (sg_0[k]^2 + sg_1[k]^2 + ..) * (1 / n_models)
 *       (MEAN);  yh[k] = fmaf(sqrt(v[k]), eps[k], yh[k]) for k < P, before s' and r are formed (the cost is never sampled);
 *       eps[k] = noise_in[e * P + k] when noise_in is given (the same at every step), else the standard normal
 *       osrl_rng's normal_word(Philox4x32-10(counter {episode_base + e, the episode's own step, k >> 2, 16}, key *seed), k & 3):
 *       a function of (seed, episode id, step, column) alone.  sample == 0: neither is read.
 * With sample == 0 and uncertainty == DISAGREEMENT the step has the bits of osrl_model_env_step on the members' first
 * od + 2 output columns. */
enum { OSRL_MODEL_ENV_UNC_DISAGREEMENT = 0, OSRL_MODEL_ENV_UNC_MAX_STD = 1 };
typedef struct {
  osrl_model_env_t env;   /* net[m].dims[n_layers] == 2 * state_dim + 3; seed is read when sample != 0 without noise_in too */
  const float* noise_in;  /* [episodes, state_dim + 1] or NULL */
  float logvar_min, logvar_max;
  int32_t sample, uncertainty;
} osrl_model_env_gauss_t;
int osrl_model_env_step_gauss(const osrl_model_env_gauss_t* env, const float* act, float* state, float* obs,
                              int32_t obs_ld, float* acc, float* unc, float* step_out, int32_t episodes, void* stream);
int osrl_model_env_collect_gauss(const osrl_model_env_gauss_t* env, const osrl_collect_t* rec, const float* act,
                                 float* state, float* obs, int32_t obs_ld, float* acc, float* unc, float* row_unc,
                                 int32_t episodes, void* stream);
/* The same four launches, pessimistic (model_env.hip, compile-time flag kPess): a rollout halts where the model stops
 * knowing, and the cost is inflated by the uncertainty.  u is the signal in use (d, or a under UNC_MAX_STD), c = yh[od + 1].
 * Per live episode e at its own step t, where the plain step forms reward and cost:
 *   cost = (cost_penalty != 0 ? fmaf(cost_penalty, u, c) : c) > 0.5 ? 1 : 0;
 *   halt = u > halt_threshold   (strict: +inf never halts, a NaN u does not halt);  on halt:
 *     r = halt_reward (it replaces the model's reward, penalty included: what acc[e][0] and the discounted sum add and
 *     what the table records), cost = halt_cost (0 or 1), the done latch acc[e][3] is set after the step is counted --
 *     the episode is finished for every later launch -- and halt_step[e] = t (left untouched otherwise; may be NULL);
 *     a recorded halting row has terminals = 1 and timeouts = 0, also when t + 1 == episode_len.
 *   The next state is written on a halting step too (state, obs, next_observations); unc[e] and row_unc include its u;
 *   sampling is unaffected.  No arithmetic of the members, the mean or the disagreement differs: with
 *   halt_threshold = +inf and cost_penalty = 0 every output has the bits of the entry point without "_halt".
 * -1 for a NaN threshold or reward, a halt_cost other than 0 / 1, a negative or non-finite cost_penalty. */
typedef struct {
  float halt_threshold, halt_reward, halt_cost, cost_penalty;
  int32_t* halt_step; /* [episodes] or NULL */
} osrl_model_env_pess_t;
int osrl_model_env_step_halt(const osrl_model_env_t* env, const osrl_model_env_pess_t* pess, const float* act,
                             float* state, float* obs, int32_t obs_ld, float* acc, float* unc, float* step_out,
                             int32_t episodes, void* stream);
int osrl_model_env_collect_halt(const osrl_model_env_t* env, const osrl_model_env_pess_t* pess,
                                const osrl_collect_t* rec, const float* act, float* state, float* obs, int32_t obs_ld,
                                float* acc, float* unc, float* row_unc, int32_t episodes, void* stream);
int osrl_model_env_step_gauss_halt(const osrl_model_env_gauss_t* env, const osrl_model_env_pess_t* pess,
                                   const float* act, float* state, float* obs, int32_t obs_ld, float* acc, float* unc,
                                   float* step_out, int32_t episodes, void* stream);
int osrl_model_env_collect_gauss_halt(const osrl_model_env_gauss_t* env, const osrl_model_env_pess_t* pess,
                                      const osrl_collect_t* rec, const float* act, float* state, float* obs,
                                      int32_t obs_ld, float* acc, float* unc, float* row_unc, int32_t episodes,
                                      void* stream);
/* Variable-length recorded rollouts made dense (compact.hip).  src / dst: the seven DSRL tables of an osrl_collect_t, whose
 * other fields are not read, episode-major with pitch episode_len in src; row_unc optional, given for both or neither.
 * len_e = (int)acc[e][2] clamped to [0, episode_len];  offsets[e] = sum_{i < e} len_i (int64 [episodes + 1], device
 * memory; offsets[episodes] = the total);  dst row offsets[e] + t = src row e * episode_len + t for t < len_e, bit for
 * bit.  Rows at and beyond offsets[episodes] of dst are not written; dst tables of episodes * episode_len rows always
 * suffice.  Out of place (src != dst).  Two launches: a one-workgroup scan, then one span per episode and table. */
int osrl_collect_compact(const osrl_collect_t* src, const float* src_row_unc, const osrl_collect_t* dst,
                         float* dst_row_unc, const float* acc, int64_t* offsets, int32_t episodes, int32_t episode_len,
                         int32_t state_dim, int32_t action_dim, void* stream);
/* Branch starts: episode e starts at row idx_e of `table` ([n_rows, state_dim], a store's observations),
 *   idx_e = umul64hi(words (x, y) of Philox4x32-10(counter {episode_base + e, 0, 0, 15}, key *seed), n)
 * (the replay gather's uniform draw; a function of (seed, episode id) alone), n = *n_rows_dev when given (a store's live
 * count: a launch follows append without a host sync), else n_rows; capped by n_rows and, when n_limit > 0, by n_limit.
 * Writes state[e], obs[e, :state_dim], start_rows[e], zeros in acc[e] and unc[e], (0, 0, 1, 0) in disc[e]. */
int osrl_model_env_branch(const float* table, int64_t n_rows, const int64_t* n_rows_dev, int64_t n_limit,
                          int32_t state_dim, const uint64_t* seed, uint32_t episode_base, float* state, float* obs,
                          int32_t obs_ld, float* acc, float* unc, float* disc /* [E,4] */,
                          int64_t* start_rows /* [E] */, int32_t episodes, void* stream);
/* Planning at act time (plan.hip, engine/mpc.py ModelPlanner): `slots` real states, `candidates` imagined episodes each;
 * episode e = n * candidates + k is candidate k of slot n.
 * osrl_plan_fanout is the reset of a planning run, in osrl_model_env_branch's place: episode e receives states[n] as its
 * model state and as obs[e, :state_dim] (columns beyond state_dim are left alone), zeros in acc[e] and unc[e], (0, 0, 1, 0)
 * in disc[e] and, where halt_step is given, halt_step[e] = -1.
 * osrl_plan_select chooses per slot among its candidates after `horizon` recorded steps.  actions: the recorder's table
 * (row e * horizon is candidate e's first action); J_k = disc[e][0] (discounted penalised return), C_k = disc[e][1]
 * (discounted cost, in the recorder's cost_scale units); T = *temperature (device memory: a captured launch follows it).
 *   valid k: neither J_k nor C_k is a NaN;   F = {valid k : C_k <= budget[n]};   n_feasible[n] = |F|.
 *   F non-empty:  k* = argmax_F J, ties to the lowest k.
 *   F empty:      k* = argmin over the valid k of C, ties to the larger J, then to the lower k;  no valid k: k* = 0.
 *   chosen[n] = k*.  action[n] = row k*, bit for bit -- unless F is non-empty and T > 0 (MPPI):
 *     w_k = (J_k == J_k* ? 1 : expf((J_k - J_k*) / T)) on F,  action[n][j] = (float)(sum_k w_k a0_k[j] / sum_k w_k), both sums
 *     in fp64 over F in ascending k by one thread (no floating-point atomics): the same inputs give the same bits.
 * 1 <= candidates <= OSRL_PLAN_MAX_CANDIDATES, slots * candidates < 2^31; -1 before any launch otherwise. */
#define OSRL_PLAN_MAX_CANDIDATES 1024
int osrl_plan_fanout(const float* states /* [slots, state_dim] */, int32_t slots, int32_t candidates, int32_t state_dim,
                     float* state, float* obs, int32_t obs_ld, float* acc, float* unc, float* disc /* [E,4] */,
                     int32_t* halt_step /* [E] or NULL */, void* stream);
int osrl_plan_select(const float* actions /* [E * horizon, action_dim] */, int32_t horizon, const float* disc /* [E,4] */,
                     const float* budget /* [slots] */, const float* temperature /* [1] */, int32_t slots,
                     int32_t candidates, int32_t action_dim, float* action /* [slots, action_dim] */,
                     int32_t* chosen /* [slots] */, int32_t* n_feasible /* [slots] */, void* stream);
/* The train step's preparation (engine/dynamics.py): xs[b] = (obs[b] - mu_s) / sd_s  [rows, state_dim];
 * target[b] = {(nobs[b] - obs[b] - mu_d) / sd_d, (rew[b] - mu_r) / sd_r, cost[b]}  [rows, state_dim + 2]. */
int osrl_dyn_prepare(const float* obs, const float* nobs, const float* rew, const float* cost, const float* mu_s,
                     const float* sd_s, const float* mu_d, const float* sd_d, const float* mu_r, const float* sd_r,
                     int32_t rows, int32_t state_dim, float* xs, float* target, void* stream);
/* The ensemble's per-member loss as a launch of its own (dyn_loss.hip): bootstrap-weighted output gradients, unweighted
 * per-row losses and the logged statistic from the members' forward outputs.  For member m, row r, target row t = target[r]:
 *   OSRL_DYN_LOSS_MSE (NL = od + 2):        l = sum_{c < od + 2} (y_c - t_c)^2,   dy_c = w 2 (y_c - t_c) scale
 *   OSRL_DYN_LOSS_GAUSS_NLL (NL = 2 od + 3): OSRL_SEED_GAUSS_NLL's expressions above with lo / hi the log-variance bounds
 *       (lo < hi), l = sum_{c < od + 1} ((y_c - t_c)^2 exp(-lv_c) + lv_c) + (y_{od+1} - t_{od+1})^2, every dy component times w.
 * The bootstrap weight w = w_m(r) is a Poisson(1) count, a function of (*boot_seed, idx[r], m) alone:
 *   word = word x of Philox4x32-10(counter {idx[r], m, 0, 17}, key = the two halves of *boot_seed),
 *   w = #{k in 0 .. 7 : word >= T_k},  T_k = floor(2^32 sum_{j <= k} e^-1 / j!) in fp64   (w in 0 .. 8, E[w] = 1 to ~1e-6).
 * idx[r] is the STORE row of batch row r, so each member sees one fixed resample of the dataset, not per-step noise; in a
 * ring store the weight belongs to the physical slot (a transition that overwrites a slot inherits the slot's weight).
 * idx == NULL: every weight is 1 (boot_seed is not read) and, for MSE, dy has the bits of OSRL_SEED_MSE's.  The loss
 * divides by the batch (scale), never by sum w; a row with w = 0 gets dy = 0 exactly (never NaN) and adds nothing to stat.
 *   row_loss[m, r] = l (UNWEIGHTED, unscaled);  weights_out[m, r] = w;  stat[0] = stat_scale sum_{m, r} w_m(r) l_m(r).
 * A row's dy, row_loss and weights_out do not depend on rows, on its position or on its neighbours.  The statistic is the
 * fixed-order sum of one partial per OSRL_DYN_LOSS_TILE rows taken by the last workgroup to arrive (no floating-point
 * atomics): two launches on the same inputs give the same bits.  With stat: partials >= ceil(rows / OSRL_DYN_LOSS_TILE)
 * floats, counter one uint32, ZERO before the first launch (re-armed by the launch); without stat neither is read.
 * n_nets <= OSRL_MAX_NETS, state_dim <= OSRL_MODEL_ENV_MAX_STATE, rows >= 1, at least one output; -1 before any launch
 * otherwise.  HOST struct; the launch goes through the argument arena (osrl_args_begin) when one is recording. */
enum { OSRL_DYN_LOSS_MSE = 0, OSRL_DYN_LOSS_GAUSS_NLL = 1 };
#define OSRL_DYN_LOSS_TILE 4
typedef struct {
  const float* y;            /* [n_nets, rows, NL]  the forward launch's output layout */
  const float* target;       /* [rows, od + 2]      osrl_dyn_prepare's table */
  const int32_t* idx;        /* [rows] store row of each batch row; NULL: every weight is 1 */
  const uint64_t* boot_seed; /* device word, read only when idx != NULL */
  float* dy;                 /* [n_nets, rows, NL] or NULL */
  float* row_loss;           /* [n_nets, rows] or NULL */
  float* weights_out;        /* [n_nets, rows] or NULL (tests, diagnostics) */
  float* stat;               /* [1] or NULL */
  float* partials;
  uint32_t* counter;
  int32_t n_nets, rows, state_dim, kind;
  float lo, hi, scale, stat_scale;
} osrl_dyn_loss_t;
int osrl_dyn_member_loss(const osrl_dyn_loss_t* d, void* stream);

/* Diagnostics (diag.hip): where the HIP runtime of this process keeps kernel arguments -- *where = 1 device memory,
 * 0 host memory (every wave then fetches its launch arguments over PCIe; see osrl_args_begin), -1 unknown.  dev_scratch:
 * 8 bytes of device memory.  Synchronises `stream`; not for the hot path. */
int osrl_kernarg_probe(uint64_t* dev_scratch, int32_t* where, uint64_t* address, void* stream);
/* (new, diagnostics) out[0] = the device's constant 100 MHz real-time counter when this one-lane launch executes.
 * Asynchronous, hipGraph-capturable: two of them around a launch of a captured step give that launch's duration inside
 * the replayed graph (bench.py `roofline.frac`; torch has no counterpart: its events cannot be timed inside a capture). */
int osrl_stamp_realtime(uint64_t* out, void* stream);

const char* osrl_version(void);

#ifdef __cplusplus
}
#endif
#endif /* OSRL_AMD_H */
