// ace_host.cpp -- host-only entry points of the C ABI (no GPU, no context):
// the optimizer steps, norm clipping, the natural-cubic-spline basis and the
// data normalisation.  They run once per iteration on P <= 818 doubles or
// once per fit, so they stay on the host.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/ace_hip.h"

namespace {

bool all_finite(int64_t P, const double *g) {
  for (int64_t j = 0; j < P; ++j)
    if (!std::isfinite(g[j])) return false;
  return true;
}

}  // namespace

extern "C" {

// Nesterov_cpp (src/optimizer_cpp.cpp:8-20)
int ace_nesterov(int64_t P, double learn_rate, double momentum, double *nu, const double *grad,
                 double *para) {
  const bool ok = all_finite(P, grad);
  for (int64_t j = 0; j < P; ++j) {
    nu[j] = momentum * nu[j] + learn_rate * grad[j];
    para[j] = para[j] + nu[j];
  }
  return ok ? 1 : 0;
}

// Nadam_cpp (src/optimizer_cpp.cpp:23-42): the Nesterov term uses the
// already-updated m (Q8).
int ace_nadam(int64_t P, double iter, double learn_rate, double beta1, double beta2, double eps,
              double *m, double *v, const double *grad, double *para) {
  const bool ok = all_finite(P, grad);
  const double c1 = 1 - std::pow(beta1, iter), c2 = 1 - std::pow(beta2, iter);
  for (int64_t j = 0; j < P; ++j) {
    m[j] = beta1 * m[j] + (1 - beta1) * grad[j];
    v[j] = beta2 * v[j] + (1 - beta2) * std::pow(grad[j], 2);
    para[j] = para[j] + learn_rate * ((beta1 * m[j] + (1 - beta1) * grad[j]) / c1) /
                            (std::sqrt(v[j] / c2) + eps);
  }
  return ok ? 1 : 0;
}

// Adam_cpp (src/optimizer_cpp.cpp:45-63)
int ace_adam(int64_t P, double iter, double learn_rate, double beta1, double beta2, double eps,
             double *m, double *v, const double *grad, double *para) {
  const bool ok = all_finite(P, grad);
  const double c1 = 1 - std::pow(beta1, iter), c2 = 1 - std::pow(beta2, iter);
  for (int64_t j = 0; j < P; ++j) {
    m[j] = (beta1 * m[j]) + (1 - beta1) * grad[j];
    v[j] = beta2 * v[j] + (1 - beta2) * std::pow(grad[j], 2);
    para[j] = para[j] + learn_rate * (m[j] / c1) / (std::sqrt(v[j] / c2) + eps);
  }
  return ok ? 1 : 0;
}

// norm_clip_cpp (src/utilities_cpp.cpp:121-129), Q5
void ace_norm_clip(int flag, int64_t P, double *grads, double max_length) {
  if (!flag) return;
  double ss = 0.0;
  for (int64_t j = 0; j < P; ++j) ss += grads[j] * grads[j];
  const double L2 = std::sqrt(ss);
  if ((L2 > max_length) && std::isfinite(L2) && (L2 != 0)) {
    for (int64_t j = 0; j < P; ++j) grads[j] = grads[j] / L2;
  }
}

// generate_ncs_matrix / generate_ncs_derivative_matrix (src/ncs_basis_cpp.cpp:5-58)
static void ncs_columns(int64_t n, const double *x, const std::vector<double> &kn, bool deriv,
                        double *out /* n x (K-1), ld n */) {
  const int64_t K = (int64_t)kn.size();
  std::vector<double> d((size_t)(n * K), 0.0);
  auto f = [&](double xv, double k) {
    const double gt = (xv > k) ? 1.0 : 0.0;
    return deriv ? 3 * gt * std::pow(xv - k, 2) : gt * std::pow(xv - k, 3);
  };
  for (int64_t r = 0; r < n; ++r) d[r + (K - 1) * n] = f(x[r], kn[K - 1]);
  for (int64_t i = 0; i < K - 1; ++i)
    for (int64_t r = 0; r < n; ++r)
      d[r + i * n] = (f(x[r], kn[i]) - d[r + (K - 1) * n]) / (kn[K - 1] - kn[i]);
  for (int64_t r = 0; r < n; ++r) d[r + (K - 1) * n] = 0.0;
  for (int64_t i = 0; i < K - 2; ++i)
    for (int64_t r = 0; r < n; ++r) out[r + i * n] = d[r + i * n] - d[r + (K - 2) * n];
  for (int64_t r = 0; r < n; ++r) out[r + (K - 2) * n] = -d[r + (K - 2) * n];
}

static int ncs_common(int64_t n, const double *x, int64_t nknots, const double *knots,
                      double *design, int64_t *ncols, bool deriv) {
  if (n < 0 || nknots < 2 || !x || !knots || !design) return ACE_ERR_ARG;
  std::vector<double> kn(knots, knots + nknots);
  std::sort(kn.begin(), kn.end());
  kn.erase(std::unique(kn.begin(), kn.end()), kn.end());
  const int64_t K = (int64_t)kn.size();
  if (K < 2) return ACE_ERR_ARG;
  for (int64_t r = 0; r < n; ++r) design[r] = deriv ? 1.0 : x[r];
  ncs_columns(n, x, kn, deriv, design + n);
  if (ncols) *ncols = K;
  return ACE_OK;
}

// ncs_basis (src/ncs_basis_cpp.cpp:61-79)
int ace_ncs_basis(int64_t n, const double *x, int64_t nknots, const double *knots,
                  double *design, int64_t *ncols) {
  return ncs_common(n, x, nknots, knots, design, ncols, false);
}

// ncs_basis_deriv (src/ncs_basis_cpp.cpp:82-99)
int ace_ncs_basis_deriv(int64_t n, const double *x, int64_t nknots, const double *knots,
                        double *design, int64_t *ncols) {
  return ncs_common(n, x, nknots, knots, design, ncols, true);
}

static double median_of(const double *p, int64_t n) {
  std::vector<double> v(p, p + n);
  std::sort(v.begin(), v.end());
  if (n % 2) return v[(size_t)(n / 2)];
  return (v[(size_t)(n / 2 - 1)] + v[(size_t)(n / 2)]) / 2.0;
}

static void unique_minmax(const double *p, int64_t n, int64_t *count, double *mn, double *mx) {
  std::vector<double> v(p, p + n);
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
  *count = (int64_t)v.size();
  *mn = v.empty() ? 0.0 : v.front();
  *mx = v.empty() ? 0.0 : v.back();
}

// normalize_train (src/utilities_cpp.cpp:13-104).  Quirks kept: binary
// columns store their location/scale in row i (not i+1) of the moments, a
// constant Z column zeroes Z.col(i) with the X-offset index, and the Z
// rescale tests isbinary(i - px - 1) (X's flags).
int ace_normalize_train(int64_t n, int px, int pz, double *y, double *X, double *Z,
                        double *mom) {
  if (n < 2 || px < 0 || pz < 0) return ACE_ERR_ARG;
  const int64_t mr = 1 + px + pz;
  auto M = [&](int64_t r, int c) -> double & { return mom[r + c * mr]; };
  for (int64_t r = 0; r < mr; ++r) {
    M(r, 0) = 0.0;
    M(r, 1) = 1.0;
    M(r, 2) = 0.0;
  }
  std::vector<int> isb((size_t)(px + pz), 0);
  for (int i = 0; i < px; ++i) {
    double *col = X + (int64_t)i * n;
    int64_t cnt;
    double mn, mx;
    unique_minmax(col, n, &cnt, &mn, &mx);
    if (cnt == 2) {
      isb[i] = 1;
      M(i + 1, 2) = 1;
      if (mn != 0) M(i, 0) = mn;
      if (mx != 1) M(i, 1) = (mx - mn);
      for (int64_t r = 0; r < n; ++r) col[r] -= M(i, 0);
      for (int64_t r = 0; r < n; ++r) col[r] /= M(i, 1);
    } else if (cnt == 1) {
      for (int64_t r = 0; r < n; ++r) col[r] = 0.0;
    }
  }
  for (int i = px; i < px + pz; ++i) {
    double *col = Z + (int64_t)(i - px) * n;
    int64_t cnt;
    double mn, mx;
    unique_minmax(col, n, &cnt, &mn, &mx);
    if (cnt == 2) {
      isb[i] = 1;
      M(i + 1, 2) = 1;
      if (mn != 0) M(i, 0) = mn;
      if (mx != 1) M(i, 1) = (mx - mn);
      for (int64_t r = 0; r < n; ++r) col[r] -= M(i, 0);
      for (int64_t r = 0; r < n; ++r) col[r] /= M(i, 1);
    } else if (cnt == 1) {
      if (i >= pz) return ACE_ERR_ARG;  // Z.col(i) out of bounds in the reference
      double *zc = Z + (int64_t)i * n;
      for (int64_t r = 0; r < n; ++r) zc[r] = 0.0;
    }
  }
  double s = 0.0;
  for (int64_t r = 0; r < n; ++r) s += y[r];
  M(0, 0) = s / (double)n;
  for (int64_t r = 0; r < n; ++r) y[r] = y[r] - M(0, 0);
  for (int i = 1; i < px + 1; ++i)
    if (isb[i - 1] == 0) {
      double *col = X + (int64_t)(i - 1) * n;
      M(i, 0) = median_of(col, n);
      for (int64_t r = 0; r < n; ++r) col[r] -= M(i, 0);
    }
  for (int i = px + 1; i < px + pz + 1; ++i)
    if (isb[i - 1] == 0) {
      double *col = Z + (int64_t)(i - px - 1) * n;
      M(i, 0) = median_of(col, n);
      for (int64_t r = 0; r < n; ++r) col[r] -= M(i, 0);
    }
  double mean = 0.0;
  for (int64_t r = 0; r < n; ++r) mean += y[r];
  mean /= (double)n;
  double ss = 0.0;
  for (int64_t r = 0; r < n; ++r) ss += (y[r] - mean) * (y[r] - mean);
  M(0, 1) = std::sqrt(ss / (double)(n - 1));
  for (int64_t r = 0; r < n; ++r) y[r] = y[r] / M(0, 1);
  for (int i = 1; i < px + 1; ++i)
    if (isb[i - 1] == 0) {
      double *col = X + (int64_t)(i - 1) * n;
      double mx = 0.0;
      for (int64_t r = 0; r < n; ++r) mx = std::max(mx, std::fabs(col[r]));
      M(i, 1) = mx;
      for (int64_t r = 0; r < n; ++r) col[r] /= M(i, 1);
    }
  for (int i = px + 1; i < px + pz + 1; ++i)
    if (i - px - 1 < (int)isb.size() && isb[i - px - 1] == 0) {
      double *col = Z + (int64_t)(i - px - 1) * n;
      double mx = 0.0;
      for (int64_t r = 0; r < n; ++r) mx = std::max(mx, std::fabs(col[r]));
      M(i, 1) = mx;
      for (int64_t r = 0; r < n; ++r) col[r] = col[r] / M(i, 1);
    }
  return ACE_OK;
}

// normalize_test (src/utilities_cpp.cpp:108-118)
int ace_normalize_test(int64_t n, int px, int pz, double *X, double *Z, const double *mom,
                       int64_t mr) {
  if (mr < 1 + px + pz) return ACE_ERR_ARG;
  for (int i = 0; i < px; ++i)
    for (int64_t r = 0; r < n; ++r)
      X[r + i * n] = (X[r + i * n] - mom[(i + 1)]) / mom[(i + 1) + mr];
  for (int i = 0; i < pz; ++i)
    for (int64_t r = 0; r < n; ++r)
      Z[r + i * n] = (Z[r + i * n] - mom[(i + 1 + px)]) / mom[(i + 1 + px) + mr];
  return ACE_OK;
}

// robust_treatment's discard levels (R/robust_treatment.R:83-84, 94):
// quantile.list = seq(0, 1, 1 / n.steps), discard.steps = R's default
// (type 7) quantile of var, idx[, t] = var <= discard.steps[t]
int ace_robust_levels(int64_t nx, const double *var, int n_steps, double *thresholds,
                      int32_t *level) {
  if (nx < 1 || !var || !thresholds || !level || n_steps < 1 || n_steps > 31) return ACE_ERR_ARG;
  if (!all_finite(nx, var)) return ACE_ERR_NONFINITE;
  std::vector<double> x(var, var + nx);
  std::sort(x.begin(), x.end());
  const double by = 1.0 / n_steps;
  for (int t = 0; t <= n_steps; ++t) {
    const double p = std::min(t * by, 1.0);
    const double index = 1 + (double)(nx - 1) * p;
    const double lo = std::floor(index), hi = std::ceil(index);
    double q = x[(size_t)lo - 1];
    const double xh = x[(size_t)hi - 1];
    if (index > lo && xh != q) {
      const double h = index - lo;
      q = (1 - h) * q + h * xh;
    }
    thresholds[t] = q;
  }
  for (int64_t i = 0; i < nx; ++i) {
    int t = 0;
    while (t < n_steps && !(var[i] <= thresholds[t])) ++t;
    level[i] = t;
  }
  return ACE_OK;
}

// The zero-pattern order of the basis and its per-block slice masks (the pair
// kernels' slice skip): a point's pattern is the set of columns of
// Z where it is nonzero (both signs of zero are zero); the points are sorted
// by the pattern's size, then by the pattern, and equal patterns keep their
// input order, so a Z without exact zeros gives the identity.
int ace_zero_pattern_order(int64_t n, int ZS, const double *Z, int64_t *perm, uint32_t *blockmask,
                           int32_t *has_mask) {
  if (n < 1 || ZS < 0 || (ZS > 0 && !Z) || !perm) return ACE_ERR_ARG;
  const int W = (ZS + 63) / 64 > 0 ? (ZS + 63) / 64 : 1;  // pattern words
  std::vector<uint64_t> pat((size_t)n * W, 0);
  std::vector<int> cnt((size_t)n, 0);
  for (int b = 0; b < ZS; ++b)
    for (int64_t r = 0; r < n; ++r)
      if (Z[r + (int64_t)b * n] != 0.0) {
        pat[(size_t)r * W + b / 64] |= (uint64_t)1 << (b % 64);
        ++cnt[(size_t)r];
      }
  for (int64_t r = 0; r < n; ++r) perm[r] = r;
  std::stable_sort(perm, perm + n, [&](int64_t a, int64_t c) {
    if (cnt[(size_t)a] != cnt[(size_t)c]) return cnt[(size_t)a] < cnt[(size_t)c];
    for (int w = W - 1; w >= 0; --w)
      if (pat[(size_t)a * W + w] != pat[(size_t)c * W + w])
        return pat[(size_t)a * W + w] < pat[(size_t)c * W + w];
    return false;
  });
  const bool mask = ZS <= 32 && blockmask != nullptr;
  if (has_mask) *has_mask = mask ? 1 : 0;
  if (!mask) return ACE_OK;
  const uint32_t all = ZS >= 32 ? 0xffffffffu : ((uint32_t)1 << ZS) - 1;
  const int64_t nblk = (n + 63) / 64;
  for (int64_t k = 0; k < nblk; ++k) {
    uint32_t m = 0;
    if (64 * (k + 1) > n) m = all;  // padding points in the block: every slice
    else
      for (int64_t j = 64 * k; j < 64 * (k + 1); ++j) m |= (uint32_t)pat[(size_t)perm[j] * W];
    blockmask[k] = m;
  }
  return ACE_OK;
}

// A coefficient posterior contracted with nz weight rows: the tails of
// pred_cpp / pred_marginal_cpp (src/pred_cpp.cpp:20-29, 70-78) at every
// (point c, row j), output index c + nx j
int ace_coef_contract(int64_t nx, int B, int64_t nz, const double *mean, const double *cov,
                      const double *W, double offset, double scale, double shift, double noise,
                      double *map, double *ci, double *var) {
  if (nx < 1 || nz < 1 || B < 1 || !mean || !cov || !W || !map || !ci || !var) return ACE_ERR_ARG;
  const int64_t N = nx * nz;
  std::vector<double> wj((size_t)B);
  for (int64_t j = 0; j < nz; ++j) {
    for (int b = 0; b < B; ++b) wj[(size_t)b] = W[j + nz * b];
    for (int64_t c = 0; c < nx; ++c) {
      double a = 0.0, q = 0.0;
      for (int b = 0; b < B; ++b) a += wj[(size_t)b] * mean[c + nx * b];
      for (int b2 = 0; b2 < B; ++b2) {
        double t = 0.0;
        for (int b = 0; b < B; ++b) t += wj[(size_t)b] * cov[c + nx * (b + (int64_t)B * b2)];
        q += t * wj[(size_t)b2];
      }
      const int64_t e = c + nx * j;
      const double yx = offset + scale * (a + shift);
      const double sd = scale * std::sqrt(std::fabs(q + noise));
      map[e] = yx;
      ci[e] = yx - 1.96 * sd;
      ci[e + N] = yx + 1.96 * sd;
      var[e] = std::pow(sd, 2);
    }
  }
  return ACE_OK;
}

// A group-summed coefficient posterior (ace_model_coef_groups) contracted with
// nz weight rows into group averages: ace_coef_contract's tail per (group g,
// row j) on gmean_g / |g| and the diagonal block C_gg / |g|^2, output index
// g + G j; cov (optional) the signed scale^2 W_j^T C_gg W_j' / |g|^2.  An
// empty group divides 0 by 0: NaN, as marginal_averages gives it.
int ace_coef_group_contract(int G, int B, int64_t nz, const double *gmean, const double *gcov,
                            const int64_t *gcount, const double *W, double offset, double scale,
                            double shift, double *map, double *ci, double *var, double *cov) {
  if (G < 1 || nz < 1 || B < 1 || !gmean || !gcov || !gcount || !W || !map || !ci || !var)
    return ACE_ERR_ARG;
  const int64_t N = (int64_t)G * nz, GB = (int64_t)G * B;
  std::vector<double> t((size_t)(nz * B));  // t[j + nz b'] = sum_b W_j[b] C_gg[b][b']
  for (int g = 0; g < G; ++g) {
    const double cnt = (double)gcount[g];
    for (int64_t j = 0; j < nz; ++j)
      for (int b2 = 0; b2 < B; ++b2) {
        double s = 0.0;
        for (int b = 0; b < B; ++b)
          s += W[j + nz * b] * gcov[(g + (int64_t)G * b) + GB * (g + (int64_t)G * b2)];
        t[(size_t)(j + nz * b2)] = s;
      }
    for (int64_t j = 0; j < nz; ++j) {
      double a = 0.0, q = 0.0;
      for (int b = 0; b < B; ++b) a += W[j + nz * b] * gmean[g + (int64_t)G * b];
      for (int b2 = 0; b2 < B; ++b2) q += t[(size_t)(j + nz * b2)] * W[j + nz * b2];
      const int64_t e = g + (int64_t)G * j;
      const double yx = offset + scale * (a / cnt + shift);
      const double sd = scale * std::sqrt(std::fabs(q)) / cnt;
      map[e] = yx;
      ci[e] = yx - 1.96 * sd;
      ci[e + N] = yx + 1.96 * sd;
      var[e] = std::pow(sd, 2);
      if (!cov) continue;
      for (int64_t j2 = 0; j2 <= j; ++j2) {  // the lower half, mirrored: exactly symmetric
        double q2 = 0.0;
        for (int b2 = 0; b2 < B; ++b2) q2 += t[(size_t)(j + nz * b2)] * W[j2 + nz * b2];
        const double c = (scale * scale) * q2 / (cnt * cnt);
        cov[g + (int64_t)G * (j + nz * j2)] = c;
        cov[g + (int64_t)G * (j2 + nz * j)] = c;
      }
    }
  }
  return ACE_OK;
}

}  // extern "C"
