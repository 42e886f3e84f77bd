// ace_batch.cpp -- host side of the batched engine (ace_batch_* of
// include/ace_hip.h): per-model data slots, the scratch matrices, and the
// training loop that enqueues k_batch_eval + k_batch_step pairs
// (ace_batch.hip), and batched prediction (ace_predict_batch,
// ace_predict_marginal_batch, ace_set_inverse_batch; ace_batch_predict.hip,
// DESIGN §16).
#include <algorithm>

#include "ace_batch.h"
#include "ace_common.h"

struct ace_batch {
  ace_ctx *ctx = nullptr;
  Shape s;       // s.PM is the batch kernels' own bucket
  int P = 0;
  int64_t M = 0, nmax = 0, ld = 0, ldo = 0;
  std::vector<int> n;          // rows per model, 0: no data yet
  std::vector<double> std_y;
  DBuf dn, dstd, y, X, Z, LZ;  // per-model slots of nmax rows
  DBuf A, A2;                  // scratch matrices: the resident inverses; the final train stats'
  DBuf theta, out;
  bool meta_dirty = true;      // dn / dstd behind the host copies
  bool has_inverse = false;
  // prediction: per model, the non-positive-definite word of its own last
  // para_update (0 / 1; 0 after ace_set_inverse_batch), and whether its
  // inverse was installed from the host since its last set_data
  DBuf dflag;
  std::vector<char> installed;
};

namespace {

void need_bytes(ace_ctx *ctx, double bytes) {
  if (bytes < 4e12) return;  // beyond any device: an overflowing size never reaches hipMalloc
  ctx->err = "ace_batch: allocation does not fit";
  throw Fail{ACE_ERR_OOM};
}

BatchView view_of(ace_batch *b, double *A, const double *theta, int64_t ldt, const int *ctl, int skip,
                  int use_mu) {
  BatchView v;
  v.M = (int)b->M;
  v.nmax = (int)b->nmax;
  v.p = b->s.p;
  v.B = b->s.B;
  v.PM = b->s.PM;
  v.ZS = b->s.ZS;
  v.P = b->P;
  v.ld = b->ld;
  v.n = b->dn.i();
  v.y = b->y.d();
  v.X = b->X.d();
  v.Z = b->Z.d();
  v.LZ = b->LZ.d();
  v.std_y = b->dstd.d();
  v.A = A;
  v.theta = theta;
  v.ldt = ldt;
  v.out = b->out.d();
  v.ldo = b->ldo;
  v.ctl = ctl;
  v.skip = skip;
  v.use_mu = use_mu;
  return v;
}

void ready(ace_batch *b) {
  ace_ctx *ctx = b->ctx;
  for (int64_t j = 0; j < b->M; ++j) arg(ctx, b->n[(size_t)j] > 0, "ace_batch_set_data() not called for every model");
  if (!b->meta_dirty) return;
  upload_bytes(ctx, b->dn.p, b->n.data(), b->n.size() * sizeof(int), "upload n");
  upload_bytes(ctx, b->dstd.p, b->std_y.data(), b->std_y.size() * sizeof(double), "upload std_y");
  b->meta_dirty = false;
}

// the result rows' non-positive-definite words into dflag: a model the train
// loop skips keeps the word of its own last para_update there
void keep_flags(ace_batch *b) {
  ck(b->ctx,
     hipMemcpy2DAsync(b->dflag.p, sizeof(double), b->out.d() + b->P + 3, (size_t)b->ldo * sizeof(double),
                      sizeof(double), (size_t)b->M, hipMemcpyDeviceToDevice, b->ctx->stream),
     "keep flags");
}

// The packed test side of a batched prediction on the device, the launch, and
// the per-point sums back on the host: res = [a | kd | q] (N each), gcov (3 M).
struct PredBatchArgs {
  const double *theta, *X2, *Zt, *Z_x;
  const int64_t *off;
  bool marginal;
  int ate;
};

void predict_batch_run(ace_batch *b, const PredBatchArgs &q, std::vector<double> &res,
                       std::vector<double> &gcov) {
  ace_ctx *ctx = b->ctx;
  const Shape &s = b->s;
  const int64_t M = b->M;
  arg(ctx, q.theta && q.off && (s.p == 0 || q.X2) && (s.B == 1 || q.Zt), "null argument");
  arg(ctx, q.off[0] == 0, "off[0] must be 0");
  for (int64_t j = 0; j < M; ++j)
    arg(ctx, q.off[j + 1] > q.off[j] && q.off[j + 1] - q.off[j] < (int64_t(1) << 30),
        "off must increase: every model needs nx_j >= 1 test points");
  ready(b);
  for (int64_t j = 0; j < M; ++j)
    arg(ctx, b->has_inverse || b->installed[(size_t)j],
        "no resident inverse: call ace_batch_para_update() or ace_set_inverse_batch() first");
  const int64_t N = q.off[M];
  if (q.ate)
    for (int64_t i = 0; i < N; ++i)
      arg(ctx, q.Z_x[i] == 0.0 || q.Z_x[i] == 1.0, "Z_x must be 0 or 1 (binary treatment)");
  need_bytes(ctx, (double)N * (s.PM + 2.0 * s.ZS + 4.0) * 8.0);
  std::vector<double> xr((size_t)(N * s.PM), 0.0), zr((size_t)(N * s.ZS), 0.0);
  for (int64_t j = 0; j < M; ++j) {
    const int64_t o = q.off[j], nx = q.off[j + 1] - o;
    if (s.p > 0) {
      std::vector<double> t = pack_rows(q.X2 + o * s.p, nx, s.p, s.PM);
      std::copy(t.begin(), t.end(), xr.begin() + o * s.PM);
    }
    if (s.B > 1) {
      std::vector<double> t = pack_rows(q.Zt + o * (s.B - 1), nx, s.B - 1, s.ZS);
      std::copy(t.begin(), t.end(), zr.begin() + o * s.ZS);
    }
  }
  DBuf dX, dZ, dLZ, dzx, doff, dres;
  upload(ctx, dX, xr.data(), xr.size(), "upload X2");
  upload(ctx, dZ, zr.data(), zr.size(), "upload Z2");
  alloc(ctx, dLZ, zr.size() * sizeof(double), "alloc log|Z2|");
  if (s.kind == ACE_KERNEL_SE)
    ck(ctx, launch_log_abs(dZ.d(), dLZ.d(), (int64_t)zr.size(), ctx->stream), "log_abs");
  if (q.ate) upload(ctx, dzx, q.Z_x, (size_t)N, "upload Z_x");
  alloc(ctx, doff, (size_t)(M + 1) * sizeof(int64_t), "alloc off");
  upload_bytes(ctx, doff.p, q.off, (size_t)(M + 1) * sizeof(int64_t), "upload off");
  upload_bytes(ctx, b->theta.p, q.theta, (size_t)(M * b->P) * sizeof(double), "upload theta");
  alloc(ctx, dres, (size_t)(3 * N + 3 * M) * sizeof(double), "alloc results");
  BatchPredView v;
  v.M = (int)M;
  v.nmax = (int)b->nmax;
  v.p = s.p;
  v.B = s.B;
  v.PM = s.PM;
  v.ZS = s.ZS;
  v.marginal = q.marginal ? 1 : 0;
  v.ate = q.ate ? 1 : 0;
  v.ld = b->ld;
  v.n = b->dn.i();
  v.y = b->y.d();
  v.X = b->X.d();
  v.Z = b->Z.d();
  v.LZ = b->LZ.d();
  v.A = b->A.d();
  v.flag = b->dflag.d();
  v.theta = b->theta.d();
  v.ldt = b->P;
  v.off = static_cast<const int64_t *>(doff.p);
  v.X2 = dX.d();
  v.Z2 = dZ.d();
  v.LZ2 = dLZ.d();
  v.zx = q.ate ? dzx.d() : nullptr;
  v.a = dres.d();
  v.kd = dres.d() + N;
  v.q = dres.d() + 2 * N;
  v.gcov = dres.d() + 3 * N;
  ck(ctx, launch_batch_predict(s.kind, v, ctx->stream), "batch predict");
  res.resize((size_t)(3 * N));
  gcov.assign((size_t)(3 * M), 0.0);
  download(ctx, res.data(), dres.d(), res.size(), "download sums");
  if (q.ate) download(ctx, gcov.data(), dres.d() + 3 * N, gcov.size(), "download group sums");
  sync(ctx);
}

}  // namespace

extern "C" {

int ace_batch_create(ace_ctx *ctx, int kind, int64_t M, int64_t nmax, int p, int B, ace_batch **out) {
  if (!ctx || !out) return ACE_ERR_ARG;
  *out = nullptr;
  ace_batch *b = new ace_batch();
  b->ctx = ctx;
  try {
    check_usable(ctx);
    ck(ctx, hipSetDevice(ctx->device), "hipSetDevice");
    b->s = check_shape(ctx, kind, p, B);
    arg(ctx, M >= 1 && M <= 0x7fffffff, "M must be >= 1");
    arg(ctx, nmax >= 1, "nmax must be >= 1");
    if (nmax > BATCH_NMAX) {
      ctx->err = "unsupported shape: the batched engine takes models of n <= 512";
      throw Fail{ACE_ERR_UNSUPPORTED};
    }
    const Shape &s = b->s;
    b->s.PM = batch_pm_bucket(p < 1 ? 1 : p);
    if (batch_lds_bytes((int)nmax, s.B, s.PM) > LDS_MAX) {
      ctx->err = "unsupported shape: the theta tables do not fit one workgroup's LDS";
      throw Fail{ACE_ERR_UNSUPPORTED};
    }
    b->P = 2 + s.B * (s.p + 1);
    b->M = M;
    b->nmax = nmax;
    b->ld = wg_rows((int)nmax);
    b->ldo = b->P + 4;
    b->n.assign((size_t)M, 0);
    b->std_y.assign((size_t)M, 1.0);
    b->installed.assign((size_t)M, 0);
    const double dM = (double)M;
    need_bytes(ctx, dM * (double)(b->ld * b->ld) * 16.0 + dM * (double)nmax * (s.PM + 2.0 * s.ZS + 1) * 8.0);
    alloc(ctx, b->dn, (size_t)M * sizeof(int), "alloc n");
    alloc(ctx, b->dstd, (size_t)M * sizeof(double), "alloc std_y");
    alloc(ctx, b->y, (size_t)(M * nmax) * sizeof(double), "alloc y");
    alloc(ctx, b->X, (size_t)(M * nmax * s.PM) * sizeof(double), "alloc X");
    alloc(ctx, b->Z, (size_t)(M * nmax * s.ZS) * sizeof(double), "alloc Z");
    alloc(ctx, b->LZ, (size_t)(M * nmax * s.ZS) * sizeof(double), "alloc LZ");
    alloc(ctx, b->A, (size_t)(M * b->ld * b->ld) * sizeof(double), "alloc batch scratch");
    alloc(ctx, b->theta, (size_t)(M * b->P) * sizeof(double), "alloc theta");
    alloc(ctx, b->out, (size_t)(M * b->ldo) * sizeof(double), "alloc results");
    alloc(ctx, b->dflag, (size_t)M * sizeof(double), "alloc flags");
    ck(ctx, hipMemsetAsync(b->dflag.p, 0, (size_t)M * sizeof(double), ctx->stream), "memset flags");
    ck(ctx, hipMemsetAsync(b->A.p, 0, b->A.bytes, ctx->stream), "memset scratch");
    ck(ctx, hipMemsetAsync(b->LZ.p, 0, b->LZ.bytes, ctx->stream), "memset LZ");
    sync(ctx);
  } catch (const Fail &f) {
    delete b;
    return f.code;
  }
  *out = b;
  return ACE_OK;
}

void ace_batch_destroy(ace_batch *b) {
  if (!b) return;
  (void)hipSetDevice(b->ctx->device);
  delete b;
}

int ace_batch_set_data(ace_batch *b, int64_t j, int64_t n_j, const double *y, const double *X,
                       const double *Z, double std_y) {
  if (!b) return ACE_ERR_ARG;
  ace_ctx *ctx = b->ctx;
  ACE_TRY
  ck(ctx, hipSetDevice(ctx->device), "hipSetDevice");
  const Shape &s = b->s;
  arg(ctx, j >= 0 && j < b->M, "model index out of range");
  arg(ctx, n_j >= 1 && n_j <= b->nmax, "n_j must be in [1, nmax]");
  arg(ctx, y && (s.p == 0 || X) && (s.B == 1 || Z), "null argument");
  const int64_t nmax = b->nmax;
  std::vector<double> yr((size_t)nmax, 0.0);
  std::copy(y, y + n_j, yr.begin());
  std::vector<double> xr = pack_rows(X, n_j, s.p, s.PM);
  xr.resize((size_t)(nmax * s.PM), 0.0);
  std::vector<double> zr((size_t)(nmax * s.ZS), 0.0);
  if (s.B > 1) {
    std::vector<double> t = pack_rows(Z, n_j, s.B - 1, s.ZS);
    std::copy(t.begin(), t.end(), zr.begin());
  }
  upload_bytes(ctx, b->y.d() + j * nmax, yr.data(), yr.size() * sizeof(double), "upload y");
  upload_bytes(ctx, b->X.d() + j * nmax * s.PM, xr.data(), xr.size() * sizeof(double), "upload X");
  upload_bytes(ctx, b->Z.d() + j * nmax * s.ZS, zr.data(), zr.size() * sizeof(double), "upload Z");
  if (s.kind == ACE_KERNEL_SE)
    ck(ctx, launch_log_abs(b->Z.d() + j * nmax * s.ZS, b->LZ.d() + j * nmax * s.ZS, nmax * s.ZS,
                           ctx->stream),
       "log_abs");
  sync(ctx);
  b->n[(size_t)j] = (int)n_j;
  b->std_y[(size_t)j] = std_y;
  b->meta_dirty = true;
  b->has_inverse = false;
  b->installed[(size_t)j] = 0;
  return ACE_OK;
  ACE_CATCH
}

int ace_batch_para_update(ace_batch *b, int iter, double *theta, double *grad, double *stats,
                          double *mu_post) {
  if (!b) return ACE_ERR_ARG;
  ace_ctx *ctx = b->ctx;
  ACE_TRY
  if (ctx->poll && ctx->poll(ctx->poll_user)) {
    ctx->err = "interrupted";
    return ACE_ERR_INTERRUPTED;
  }
  ck(ctx, hipSetDevice(ctx->device), "hipSetDevice");
  arg(ctx, theta && grad && stats, "null argument");
  ready(b);
  const int P = b->P;
  const int64_t M = b->M;
  upload_bytes(ctx, b->theta.p, theta, (size_t)(M * P) * sizeof(double), "upload theta");
  ck(ctx, launch_batch_eval(b->s.kind, view_of(b, b->A.d(), b->theta.d(), P, nullptr, 0, iter == 1),
                            ctx->stream),
     "batch eval");
  keep_flags(b);
  std::vector<double> h((size_t)(M * b->ldo));
  download(ctx, h.data(), b->out.d(), h.size(), "download results");
  sync(ctx);
  b->has_inverse = true;
  for (int64_t j = 0; j < M; ++j) {
    const double *o = h.data() + j * b->ldo;
    std::copy(o, o + P, grad + j * P);
    stats[2 * j] = o[P];
    stats[2 * j + 1] = o[P + 1];
    if (mu_post) mu_post[j] = o[P + 2];
    if (iter == 1) theta[1 + j * P] = o[P + 2];  // mean_solution before the gradient
  }
  return ACE_OK;
  ACE_CATCH
}

int ace_batch_train(ace_batch *b, int optimizer, double learn_rate, double momentum, double beta1,
                    double beta2, int norm_clip, double clip_at, int maxiter, double tol,
                    double *theta, double *stats, int *iters, int *converged, int *status) {
  if (!b) return ACE_ERR_ARG;
  ace_ctx *ctx = b->ctx;
  ACE_TRY
  arg(ctx,
      theta && stats && iters && converged && status && maxiter >= 1 &&
          (optimizer == ACE_OPT_NESTEROV || optimizer == ACE_OPT_ADAM || optimizer == ACE_OPT_NADAM),
      "ace_batch_train: bad argument");
  ck(ctx, hipSetDevice(ctx->device), "hipSetDevice");
  ready(b);
  const int P = b->P;
  const int64_t M = b->M, ldh = 2 * (int64_t)(maxiter + 2);
  hipStream_t st = ctx->stream;
  DBuf dst, dhist, dctl;
  std::vector<double> init((size_t)(3 * P * M), 0.0);
  for (int64_t j = 0; j < M; ++j) std::copy(theta + j * P, theta + (j + 1) * P, init.begin() + j * 3 * P);
  upload(ctx, dst, init.data(), init.size(), "upload train state");
  need_bytes(ctx, (double)ldh * (double)M * 8.0);
  std::vector<double> hz((size_t)(ldh * M), 0.0);
  upload(ctx, dhist, hz.data(), hz.size(), "upload stats");
  alloc(ctx, dctl, (size_t)(2 * M) * sizeof(int), "alloc train control");
  ck(ctx, hipMemsetAsync(dctl.p, 0, (size_t)(2 * M) * sizeof(int), st), "memset control");
  BatchStepCfg c;
  c.opt = opt_cfg(optimizer, learn_rate, momentum, beta1, beta2, norm_clip, clip_at, tol);
  c.P = P;
  c.M = (int)M;
  const int K = train_sync_every();
  std::vector<int> ctl((size_t)(2 * M), 0);
  auto read_ctl = [&]() {
    sync(ctx);
    ck(ctx, hipMemcpyAsync(ctl.data(), dctl.p, ctl.size() * sizeof(int), hipMemcpyDeviceToHost, st),
       "download control");
    sync(ctx);
  };
  bool interrupted = false;
  for (int it = 1; it <= maxiter; ++it) {
    if (ctx->poll && ctx->poll(ctx->poll_user)) {  // before iteration it, like para_update
      interrupted = true;
      break;
    }
    // a stopped model is skipped by both kernels: its theta, stats and
    // resident inverse stay those of its own last para_update (Q6)
    ck(ctx, launch_batch_eval(b->s.kind, view_of(b, b->A.d(), dst.d(), 3 * P, dctl.i(), 1, it == 1), st),
       "batch eval");
    ck(ctx, launch_batch_step(c, it, b->out.d(), b->ldo, dst.d(), dhist.d(), ldh, dctl.i(), st),
       "batch step");
    b->has_inverse = true;
    if (it % K == 0 || it == maxiter) {
      read_ctl();
      bool all = true;
      for (int64_t j = 0; j < M; ++j) all = all && ctl[(size_t)(2 * j + 1)] != 0;
      if (all) break;
    }
  }
  read_ctl();
  keep_flags(b);  // before the final stats' evaluation overwrites the result rows
  bool any_ok = false;
  for (int64_t j = 0; j < M; ++j) {
    const int it = ctl[(size_t)(2 * j)], stop = ctl[(size_t)(2 * j + 1)];
    iters[j] = it;
    status[j] = stop == 2 ? ACE_ERR_NONFINITE : ACE_OK;
    converged[j] = (stop != 2 && !interrupted && it < maxiter) ? 1 : 0;
    any_ok = any_ok || stop != 2;
  }
  std::vector<double> hs(init.size());
  download(ctx, hs.data(), dst.d(), hs.size(), "download theta");
  download(ctx, stats, dhist.d(), (size_t)(ldh * M), "download stats");
  sync(ctx);
  for (int64_t j = 0; j < M; ++j) std::copy(hs.begin() + j * 3 * P, hs.begin() + j * 3 * P + P, theta + j * P);
  if (interrupted) {
    ctx->err = "interrupted";
    return ACE_ERR_INTERRUPTED;
  }
  if (any_ok) {
    // get_train_stats at each model's final theta, into the second scratch
    // set: the resident inverses are not replaced
    need_bytes(ctx, (double)M * (double)(b->ld * b->ld) * 8.0);
    alloc(ctx, b->A2, (size_t)(M * b->ld * b->ld) * sizeof(double), "alloc batch scratch 2");
    ck(ctx, launch_batch_eval(b->s.kind, view_of(b, b->A2.d(), dst.d(), 3 * P, dctl.i(), 2, 0), st),
       "batch eval");
    std::vector<double> h((size_t)(M * b->ldo));
    download(ctx, h.data(), b->out.d(), h.size(), "download results");
    sync(ctx);
    for (int64_t j = 0; j < M; ++j) {
      if (status[j] != ACE_OK) continue;
      const double *o = h.data() + j * b->ldo;
      double *sj = stats + j * ldh;
      sj[2 * (iters[j] + 1)] = o[P];
      sj[2 * (iters[j] + 1) + 1] = o[P + 1];
    }
  }
  return ACE_OK;
  ACE_CATCH
}

int ace_batch_get_inverse(ace_batch *b, int64_t j, double *inv) {
  if (!b) return ACE_ERR_ARG;
  ace_ctx *ctx = b->ctx;
  ACE_TRY
  ck(ctx, hipSetDevice(ctx->device), "hipSetDevice");
  arg(ctx, inv != nullptr, "null argument");
  arg(ctx, j >= 0 && j < b->M, "model index out of range");
  arg(ctx, (b->has_inverse || b->installed[(size_t)j]) && b->n[(size_t)j] > 0, "no para_update yet");
  const int64_t n = b->n[(size_t)j], ld = b->ld;
  std::vector<double> h((size_t)(ld * n));  // the model's first n columns hold -A^-1 (lower)
  download(ctx, h.data(), b->A.d() + j * ld * ld, h.size(), "download inverse");
  sync(ctx);
  for (int64_t c = 0; c < n; ++c)
    for (int64_t r = c; r < n; ++r) {
      const double v = -h[(size_t)(r + c * ld)];
      inv[r + c * n] = v;
      inv[c + r * n] = v;
    }
  return ACE_OK;
  ACE_CATCH
}

int ace_set_inverse_batch(ace_batch *b, int64_t j, const double *inv) {
  if (!b) return ACE_ERR_ARG;
  ace_ctx *ctx = b->ctx;
  ACE_TRY
  ck(ctx, hipSetDevice(ctx->device), "hipSetDevice");
  arg(ctx, inv != nullptr, "null argument");
  arg(ctx, j >= 0 && j < b->M, "model index out of range");
  arg(ctx, b->n[(size_t)j] > 0, "ace_batch_set_data() not called for this model");
  const int64_t n = b->n[(size_t)j], ld = b->ld;
  // the model's first n columns: -inv in the lower triangle, zero elsewhere
  // (prediction reads the n x n part only; a para_update assembles all anew)
  std::vector<double> h((size_t)(ld * n), 0.0);
  for (int64_t c = 0; c < n; ++c)
    for (int64_t r = c; r < n; ++r) h[(size_t)(r + c * ld)] = -inv[r + c * n];
  upload_bytes(ctx, b->A.d() + j * ld * ld, h.data(), h.size() * sizeof(double), "upload inverse");
  const double zero = 0.0;
  upload_bytes(ctx, b->dflag.d() + j, &zero, sizeof(double), "clear flag");
  b->installed[(size_t)j] = 1;
  return ACE_OK;
  ACE_CATCH
}

int ace_predict_batch(ace_batch *b, const double *theta, const int64_t *off, const double *X2,
                      const double *Z2, const double *mean_y, const double *std_y, double *map,
                      double *ci, double *var) {
  if (!b) return ACE_ERR_ARG;
  ace_ctx *ctx = b->ctx;
  ACE_TRY
  ck(ctx, hipSetDevice(ctx->device), "hipSetDevice");
  arg(ctx, mean_y && std_y && map && ci && var, "null argument");
  std::vector<double> res, gcov;
  predict_batch_run(b, PredBatchArgs{theta, X2, Z2, nullptr, off, false, 0}, res, gcov);
  const int64_t N = off[b->M];
  for (int64_t j = 0; j < b->M; ++j) {
    const int64_t o = off[j], nx = off[j + 1] - o;
    const double *th = theta + j * b->P;
    finish_pred(nx, res.data() + o, res.data() + N + o, res.data() + 2 * N + o, th[0], th[1],
                mean_y[j], std_y[j], map + o, ci + 2 * o, var + o);
  }
  return ACE_OK;
  ACE_CATCH
}

int ace_predict_marginal_batch(ace_batch *b, const double *theta, const int64_t *off,
                               const double *X2, const double *dZ2, const double *Z_x,
                               const double *std_y, const double *std_Z, int calculate_ate,
                               double *map, double *ci, double *var, double *avg) {
  if (!b) return ACE_ERR_ARG;
  ace_ctx *ctx = b->ctx;
  ACE_TRY
  ck(ctx, hipSetDevice(ctx->device), "hipSetDevice");
  arg(ctx, std_y && std_Z && map && ci && var, "null argument");
  arg(ctx, !calculate_ate || (Z_x && avg), "calculate_ate needs Z_x and avg");
  std::vector<double> res, gcov;
  predict_batch_run(b, PredBatchArgs{theta, X2, dZ2, Z_x, off, true, calculate_ate ? 1 : 0}, res,
                    gcov);
  const int64_t N = off[b->M];
  for (int64_t j = 0; j < b->M; ++j) {
    const int64_t o = off[j], nx = off[j + 1] - o;
    // the three quadratic forms from the two groups' covariance (g: untreated,
    // treated), summed as ace_model_robust_treatment sums its groups
    const double ctt = gcov[(size_t)(3 * j)], ctu = gcov[(size_t)(3 * j + 1)],
                 cuu = gcov[(size_t)(3 * j + 2)];
    const double post[3] = {((cuu + ctu) + ctu) + ctt, ctt, cuu};
    finish_marginal(nx, res.data() + o, res.data() + N + o, res.data() + 2 * N + o, std_y[j],
                    std_Z[j], calculate_ate ? Z_x + o : nullptr, calculate_ate ? post : nullptr,
                    map + o, ci + 2 * o, var + o, calculate_ate ? avg + 12 * j : nullptr);
  }
  return ACE_OK;
  ACE_CATCH
}

}  // extern "C"
