// loss_terms.h -- the element arithmetic of every loss, stated once: the loss kernels (glue.hip, dyn_loss.hip), the
// loss seeds of the backward launches (mlp.hip seed_dy, vae_ns.hip) and the KL rows of mlp_nb.hip call these functions, so
// a seeded launch has the loss kernel's bits by construction.
// Values in, values out: no pointers, no row loops, no reductions, no pin() -- a call site keeps its own loads, load
// groups, ragged-row selects and accumulation order.  The only functions that load are load_members / min_members.
// Everything is internal to the including translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace {

constexpr float kLogStdMin = -20.0f, kLogStdMax = 2.0f;  // net.py:148-149
constexpr float kVaeLsMin = -4.0f, kVaeLsMax = 15.0f;    // net.py:325

// ---- small ensembles ---------------------------------------------------------------------------------------------
// Ensemble outputs are [n][stride].  n <= kEns (host-checked: every reference config): all members of an element are
// requested together as straight-line code -- members past n re-read member 0 and are dropped by a select -- so the
// loads of one batch row overlap.  Same fminf order as a counted loop over the members, same bits.
constexpr int kEns = 4;
__device__ __forceinline__ void load_members(const float* __restrict__ q, int n, int stride, int i, float (&v)[kEns]) {
#pragma unroll
  for (int e = 0; e < kEns; ++e) v[e] = q[(size_t)(e < n ? e : 0) * stride + i];
}
__device__ __forceinline__ float min_members(const float* __restrict__ q, int n, int stride, int i) {
  float v[kEns];
  load_members(q, n, stride, i, v);
  float m = v[0];
#pragma unroll
  for (int e = 1; e < kEns; ++e) m = e < n ? fminf(m, v[e]) : m;
  return m;
}

// ---- scalar functions --------------------------------------------------------------------------------------------
__device__ __forceinline__ float softplus(float x) { return x > 20.0f ? x : log1pf(expf(x)); }  // F.softplus
__device__ __forceinline__ float sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
// the overflow-free form the bounded log-variance uses: softplus(x) = max(x, 0) + log1p(exp(-|x|)); its slope is sigmoid
__device__ __forceinline__ float softplus_abs(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// KL(N(mean, sd) || N(0, 1)) of one latent dimension, sd = exp(clamp(log_std))  (cpq.py:128)
__device__ __forceinline__ float kl_elem(float mean, float ls_raw) {
  const float sd = expf(fminf(fmaxf(ls_raw, kVaeLsMin), kVaeLsMax));
  return -0.5f * (1.0f + logf(sd * sd) - mean * mean - sd * sd);
}

// ---- backups -----------------------------------------------------------------------------------------------------
// r + gamma (1 - done) (qc_targ <= thres) q_targ      cpq.py:145-146
__device__ __forceinline__ float cpq_critic_backup(float rew, float done, float qt, float qct, float gamma,
                                                   float thres) {
  return rew + gamma * (1.0f - done) * (qct <= thres ? 1.0f : 0.0f) * qt;
}
__device__ __forceinline__ float cpq_cost_backup(float cost, float qc_min, float gamma) {  // cpq.py:161
  return cost + gamma * qc_min;
}
// the CPQ actor's min over the reward critics with torch's argmin (first of equals), and its constraint mask
__device__ __forceinline__ void cpq_actor_argmin(const float (&qv)[kEns], int n, float& qm, int& am) {
  qm = qv[0];
  am = 0;
#pragma unroll
  for (int e = 1; e < kEns; ++e) {
    const bool lt = e < n && qv[e] < qm;
    qm = lt ? qv[e] : qm;
    am = lt ? e : am;
  }
}
__device__ __forceinline__ float cpq_actor_mask(float qc_min, float thres) { return qc_min <= thres ? 1.0f : 0.0f; }
// BCQ's clipped double Q over the two target groups' minima (bcql.py:146-148) and the backup over the best sample
__device__ __forceinline__ float bcq_mix(float q1, float q2, float lmbda) {
  return lmbda * fminf(q1, q2) + (1.0f - lmbda) * fmaxf(q1, q2);
}
__device__ __forceinline__ float bcq_backup(float base, float nd, float best, float gamma) {
  return base + gamma * nd * best;
}
__device__ __forceinline__ float fqe_backup(float x, float done, float q_next, float gamma) {
  return x + gamma * (1.0f - done) * q_next;
}

// ---- terms and their gradients ------------------------------------------------------------------------------------
// squared error of d = y - target: the term of the sum, and d(scale * term)/dy
__device__ __forceinline__ float sq_term(float d) { return d * d; }
__device__ __forceinline__ float sq_grad(float d, float scale) { return 2.0f * d * scale; }

// PETS' soft clamp of a raw log-variance to (lo, hi): lv = lo + softplus(hi - softplus(hi - raw) - lo)
__device__ __forceinline__ float bounded_logvar(float raw, float lo, float hi) {
  const float lv1 = hi - softplus_abs(hi - raw);
  return lo + softplus_abs(lv1 - lo);
}
// Gaussian NLL of one output (d = mean - target) under that log-variance: the clamp's parts, then the term
// d^2 exp(-lv) + lv, d(scale * term)/d(mean) and d(scale * term)/d(raw).  Three functions, not one that returns all
// three: a site evaluates each where it needs it (seed_dy: the term and the mean gradient for a mean column, the raw
// gradient for a log-variance column; dyn_loss_body: all three side by side), and the compiler's fma contraction of
// d * d * iv depends on which of them share a block -- the two sites never had each other's last bit, and keep their own.
struct LogVar {
  float lv1, lv, iv;  // the inner clamp, the bounded log-variance, exp(-lv)
};
__device__ __forceinline__ LogVar gauss_nll_logvar(float raw, float lo, float hi) {
  LogVar v;
  v.lv1 = hi - softplus_abs(hi - raw);
  v.lv = lo + softplus_abs(v.lv1 - lo);
  v.iv = expf(-v.lv);
  return v;
}
__device__ __forceinline__ float gauss_nll_term(float d, const LogVar v) { return d * d * v.iv + v.lv; }
__device__ __forceinline__ float gauss_nll_g_mean(float d, const LogVar v, float scale) { return 2.0f * d * v.iv * scale; }
__device__ __forceinline__ float gauss_nll_g_raw(float d, float raw, const LogVar v, float lo, float hi, float scale) {
  return (1.0f - d * d * v.iv) * sigmoid(hi - raw) * sigmoid(v.lv1 - lo) * scale;
}

// squashed-Gaussian head backward: da = the summed dL/d(action), t = tanh(u), u = mu + exp(clamp(log_std)) eps;
// du = dL/d(mu), and from it dL/d(raw log_std) (0 outside the clamp)
__device__ __forceinline__ float gauss_head_du(float da, float max_a, float t) { return da * max_a * (1.0f - t * t); }
__device__ __forceinline__ float gauss_head_dls(float du, float lsr, float ev) {
  const float ls = fminf(fmaxf(lsr, kLogStdMin), kLogStdMax);
  const bool inside = lsr >= kLogStdMin && lsr <= kLogStdMax;
  return inside ? du * ev * expf(ls) : 0.f;
}

}  // namespace
