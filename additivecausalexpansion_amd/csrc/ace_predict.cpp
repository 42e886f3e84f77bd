// ace_predict.cpp -- what a model does with the resident inverse of its last
// para_update.  Shared: with_pred_scratch (the retained scratch and its
// out-of-memory / keep policy), PredFront (the setup every path starts with)
// and symm_resident (A^-1 V: ace_model_apply_inverse).  Paths:
//   * pred_pipeline: pred_cpp / pred_marginal_cpp with ATE / ATT / ATU over
//     abstract operands (the model's here, the handles' in ace_dmat.cpp);
//   * predict_impl, group_pass: ace_model_predict, _predict_marginal,
//     _predict_marginal_groups, _robust_treatment;
//   * coef_pass, coef_cross: ace_model_coef_posterior, _predict_surface,
//     _coef_cross;
//   * coef_group_pass: ace_model_coef_groups, _average_response;
//   * joint_pass: ace_model_predict_joint (and ace_potrf_lower beside it).
//
// The reference's predict path (R/kernel_SE_R6.R:75-97) builds K_xX and
// K_xx (or their n x n2 x B "elements" cubes) on the host, ships the stored
// invKmatn, and pred_cpp / pred_marginal_cpp (src/pred_cpp.cpp:8-126) form
// tmp = K_xX invK_XX with a full GEMM and the full n2 x n2 matrix
// K_xx - tmp K_xX^T, of which only the diagonal (and, for ATE/ATT/ATU,
// three quadratic forms) is used.  Here:
//   * the inverse is the one the last para_update left in HBM (Q6: the
//     theta_{T-1} inverse with kernels at the caller's theta_T), read from
//     the swept matrix's lower triangle (-A^-1) by k_symm -- never copied,
//     never sent to the host;
//   * K_xX (the marginal slice sum for predict_marginal) is assembled on the
//     device, test points in chunks, and T' = A^-1 K_xX^T (n x chunk) is one
//     MFMA product per chunk;
//   * only diag(K_xx) is formed (r2 = 0: launch_kdiag), and the ATE/ATT/ATU
//     quadratic forms use Km_xx (n2 x n2) and three n-vectors;
//   * sharded models: each rank multiplies by the inverse entries it stores
//     and the per-test-point sums are all-reduced (2 n2 + 3 doubles), never
//     the n x n2 products.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cmath>
#include <functional>
#include <vector>

#include "../../include/ace_hip.h"

#include "ace_common.h"
#include "ace_internal.h"
#include "ace_model.h"
#include "ace_retry.h"

using namespace ace;

namespace {

// test points per chunk: K_xX and T' are n x 8192 each (4.3 GB at n = 65536)
constexpr int64_t NXC = 8192;

// retained scratch above this size is released after the call (n = 16384,
// nx = 4096 keeps its 1.1 GB; n = 65536 with 8192-point chunks frees 8.6 GB)
constexpr size_t PRED_KEEP_BYTES = size_t(4) << 30;

// The large buffers (K_xX, T', K_xx chunks), kept in the context between
// calls.  They carry no values from one call to the next, except the last
// chunk's K_xX from the pipeline to the grouped pass of the same call
// (KeptChunk).
struct PredScratch {
  DBuf K, T, Kxx;
};

// the context's scratch; create: make it if there is none (else null)
std::shared_ptr<PredScratch> pred_scratch(ace_ctx *ctx, bool create) {
  std::shared_ptr<PredScratch> ps = std::static_pointer_cast<PredScratch>(ctx->pred_state);
  if (!ps && create) {
    ps = std::make_shared<PredScratch>();
    ctx->pred_state = ps;
  }
  return ps;
}

void release_pred_state(ace_ctx *ctx) {
  if (auto ps = pred_scratch(ctx, false)) {
    ps->K.release();
    ps->T.release();
    ps->Kxx.release();
  }
  ctx->pred_state.reset();
}

// Runs body(PredScratch &) under the scratch policy.  The reference handed to
// the body stays valid if an allocation failure inside it drops
// ctx->pred_state (alloc): the wrapper holds the scratch for the run.  Out of
// device memory frees the scratch -- all three buffers, including the ones
// the failed run still referenced -- and the pooled sweep buffers, and the
// body runs once more on a new one (it writes its outputs only at its end).
template <class Body>
void with_pred_scratch(ace_ctx *ctx, Body &&body) {
  retry_once_on<Fail>(
      ACE_ERR_OOM,
      [&] {
        const std::shared_ptr<PredScratch> ps = pred_scratch(ctx, true);
        body(*ps);
      },
      [&] {
        (void)hipGetLastError();
        sync(ctx);  // the failed run's launches may still read the scratch
        release_pred_state(ctx);
        ctx->sweep_pool.clear();
      },
      [&] {
        if (auto ps = pred_scratch(ctx, false))
          if (ps->K.bytes + ps->T.bytes + ps->Kxx.bytes > PRED_KEEP_BYTES) release_pred_state(ctx);
      });
}

// out (n x k, ld n) = A^-1 V, summed over the simulated ranks; on an RCCL
// rank the caller all-reduces (the partial holds this rank's entries only).
void symm_resident(ace_model *m, const double *V, int64_t ldv, bool vt, int64_t k, double *out,
                   DBuf &tmp) {
  ace_ctx *ctx = m->ctx;
  hipStream_t st = ctx->stream;
  const int64_t n = m->n;
  if (!m->shard) {  // -A^-1 is stored: scale -1
    ck(ctx, launch_symm(m->sw.A.d(), m->naug, n, 1, 0, V, ldv, vt, k, -1.0, out, n, st), "symm");
    return;
  }
  const int G = shard_world(m->shard);
  for (int j = 0; j < shard_nlocal(m->shard); ++j) {
    double *dst = out;
    if (j > 0) {
      alloc(ctx, tmp, (size_t)(n * k) * sizeof(double), "alloc symm partial");
      dst = tmp.d();
    }
    ck(ctx, launch_symm(shard_A0(m->shard, j), m->naug, n, G, shard_rank_of(m->shard, j), V, ldv,
                        vt, k, -1.0, dst, n, st),
       "symm");
    if (j > 0) ck(ctx, launch_add(tmp.d(), out, n * k, st), "sim all-reduce");
  }
}

// ACE_PRED_TRI (default 1): single-GPU prediction takes the variance's
// quadratic form through the strictly lower triangle of A^-1 (half the
// MFMA work of the full symmetric product; 0 = the full product, A/B)
bool pred_tri() {
  static const bool v = env_int("ACE_PRED_TRI", 1) != 0;
  return v;
}

// What every prediction path sets up before its own work, at the caller's
// theta (Q6).  Zt = null uploads a basis of ones (the slice kernels of the
// coefficient paths do not read it; upload_side wants one).  parts: FRONT_W
// adds w = y - mu (a = tmp (y - mu) with tmp^T = T', src/pred_cpp.cpp:20, 70);
// FRONT_TRI adds, where the triangular form applies (one GPU, ACE_PRED_TRI),
// diag(A^-1) and what ainv_w needs.
enum : unsigned { FRONT_W = 1, FRONT_TRI = 2 };
struct PredFront {
  ace_model *m;
  const double mu;
  DBuf dtab, dw, ddiag, dscal;
  TabView tv{};
  SideBufs test;
  PairSide train{};
  int b0, b1;        // the slices summed: all, or the marginal ones (src/pred_cpp.cpp:55-67)
  bool tri = false;  // the triangular form: ddiag holds diag(A^-1)

  PredFront(ace_model *m_, const double *theta, int64_t nx, const double *X2, const double *Zt,
            bool marginal, unsigned parts)
      : m(m_), mu(theta[1]) {
    ace_ctx *ctx = m->ctx;
    hipStream_t st = ctx->stream;
    const Shape &s = m->s;
    const int64_t n = m->n;
    b0 = marginal && s.B > 1 ? 1 : 0;
    b1 = marginal ? (s.B > 1 ? s.B : 1) : s.B;
    std::vector<double> tab = make_tab(theta, s, false);
    upload(ctx, dtab, tab.data(), tab.size(), "upload tables");
    tv = tab_view(dtab, s);
    const std::vector<double> ones(Zt ? 0 : (size_t)(nx * s.ZS), 1.0);
    upload_side(ctx, test, s, X2, Zt ? Zt : ones.data(), nx, nx);
    train = m->shard ? shard_train_side(m->shard) : m->side.view(n);
    if (!(parts & FRONT_W)) return;
    alloc(ctx, dw, (size_t)n * sizeof(double), "alloc w");
    ck(ctx, launch_center(m->shard ? shard_train_y(m->shard) : m->y.d(), n, mu, dw.d(), st),
       "center y");
    tri = (parts & FRONT_TRI) && !m->shard && pred_tri();
    if (!tri) return;  // -A^-1 is stored: scale -1
    alloc(ctx, ddiag, (size_t)n * sizeof(double), "alloc diag");
    ck(ctx, launch_diag_scaled(m->sw.A.d(), m->naug, n, -1.0, ddiag.d(), st), "diag");
    alloc(ctx, dscal, 8 * sizeof(double), "alloc scalars");
  }
  // dst (n) = A^-1 (y - mu) = A^-1 y - mu A^-1 1: the AUG rows the sweep left
  // in A (k_alpha_from_aug with the caller's mu), no n^2 pass.  tri only.
  // A launch, not a buffer of the front: the coefficient pass issues it at
  // once, the pipeline after its own uploads.
  void ainv_w(double *dst) const {
    ck(m->ctx, launch_alpha_from_aug(m->sw.A.d(), m->naug, m->npad, m->n, mu, 0, dst, dscal.d(),
                                     m->ctx->stream, nullptr),
       "A^-1 w");
  }
};

void pipeline_body(const PredOps &op, const PredReq &rq, PredScratch &ps) {
  ace_ctx *ctx = op.ctx;
  hipStream_t st = ctx->stream;
  const int64_t n = op.n, nx = rq.nx;
  const int ate = rq.ate;
  DBuf &dKc = ps.K, &dT = ps.T, &dKmxx = ps.Kxx;
  DBuf dad, dkd, dtmp, dW3, dS3, dU3, dq3, dvt, ddot;
  const int64_t chunk = std::min<int64_t>(NXC, nx);
  alloc(ctx, dT, (size_t)(chunk * n) * sizeof(double), "alloc T");
  alloc(ctx, dad, (size_t)(2 * nx) * sizeof(double), "alloc sums");  // [a | d]
  alloc(ctx, dkd, (size_t)nx * sizeof(double), "alloc diag");
  if (ate) {
    const std::vector<double> W3 = ate_weights(rq.Z_x, nx);
    upload(ctx, dW3, W3.data(), W3.size(), "upload weights");
    alloc(ctx, dS3, (size_t)(3 * n) * sizeof(double), "alloc s");
    alloc(ctx, dU3, (size_t)(3 * n) * sizeof(double), "alloc u");
    alloc(ctx, dvt, (size_t)n * sizeof(double), "alloc gemv");
    ck(ctx, launch_fill(dS3.d(), 3 * n, 0.0, st), "zero");
    ck(ctx, launch_fill(dU3.d(), 3 * n, 0.0, st), "zero");
  }
  // triangular form (op.trmm): the variance from Y = L K_xX^T, L the
  // strictly lower part of A^-1 (half of the full product's flops), the map
  // from s = A^-1 w, and u_j = A^-1 s_j once after the loop
  const bool tri = (bool)op.trmm;
  DBuf dsv;
  if (tri) {
    alloc(ctx, dsv, (size_t)n * sizeof(double), "alloc s");
    if (op.ainv_w)
      op.ainv_w(dsv.d());
    else
      op.symv(op.w, n, 1, dsv.d(), dtmp);
  }
  for (int64_t c0 = 0; c0 < nx; c0 += chunk) {
    const int64_t nc = std::min<int64_t>(chunk, nx - c0);
    int64_t ldk = 0;
    const double *Kc = op.cross(c0, nc, &ldk, dKc);  // K_xX rows c0 .. c0 + nc
    if (tri) {
      op.trmm(Kc, ldk, nc, dT.d());
      ck(ctx, launch_pred_cols_tri(dT.d(), n, Kc, ldk, n, nc, dsv.d(), op.sdiag, dad.d() + c0,
                                   dad.d() + nx + c0, st),
         "pred sums");
    } else {
      // T' = A^-1 K_xX^T (n x nc): the transpose of tmp = K_xX invK_XX
      op.symm(Kc, ldk, nc, dT.d(), dtmp);
      ck(ctx, launch_pred_cols(dT.d(), n, Kc, ldk, n, nc, op.w, dad.d() + c0, dad.d() + nx + c0, st),
         "pred sums");
    }
    if (ate)
      for (int j = 0; j < 3; ++j) {
        const double *wj = dW3.d() + j * nx + c0;
        // s_j += K_xX^T w_j, u_j += T' w_j = A^-1 K_xX^T w_j
        ck(ctx, launch_gemv_t(Kc, ldk, nc, n, wj, dvt.d(), st), "gemv_t");
        ck(ctx, launch_add(dvt.d(), dS3.d() + j * n, n, st), "add");
        if (tri) continue;
        ck(ctx, launch_gemv(dT.d(), n, n, nc, wj, dvt.d(), st), "gemv");
        ck(ctx, launch_add(dvt.d(), dU3.d() + j * n, n, st), "add");
      }
  }
  if (tri && ate) op.symv(dS3.d(), n, 3, dU3.d(), dtmp);  // u_j = A^-1 s_j
  op.kdiag(dkd.d());
  std::vector<double> q3(3, 0.0), dots(3, 0.0);
  if (ate) {
    // w_j^T Km_xx w_j with the full marginal test kernel
    int64_t ldx = 0;
    const double *Kxx = op.kxx(&ldx, dKmxx);
    alloc(ctx, dq3, (size_t)(3 * nx + 3) * sizeof(double), "alloc quad");
    ck(ctx, launch_quad3(Kxx, ldx, nx, dW3.d(), dq3.d(), st), "quad3");
    // s_j . u_j  (the rank's share of s_j^T A^-1 s_j)
    alloc(ctx, ddot, 3 * sizeof(double), "alloc dots");
    for (int j = 0; j < 3; ++j)
      ck(ctx, launch_gemv_t(dS3.d() + j * n, n, n, 1, dU3.d() + j * n, ddot.d() + j, st), "dot");
    if (op.allreduce) op.allreduce(ddot.d(), 3);
    download(ctx, q3.data(), dq3.d(), 3, "download quad");
    download(ctx, dots.data(), ddot.d(), 3, "download dots");
  }
  if (op.allreduce) op.allreduce(dad.d(), 2 * nx);
  std::vector<double> ad((size_t)(2 * nx)), kd((size_t)nx);
  download(ctx, ad.data(), dad.d(), ad.size(), "download sums");
  download(ctx, kd.data(), dkd.d(), kd.size(), "download diag");
  sync(ctx);
  if (!rq.marginal) {
    finish_pred(nx, ad.data(), kd.data(), ad.data() + nx, rq.sigma, rq.mu, rq.mean_y, rq.std_y,
                rq.map, rq.ci, rq.var);
    return;
  }
  std::vector<double> post(3);
  for (int j = 0; j < 3; ++j) post[(size_t)j] = q3[(size_t)j] - dots[(size_t)j];
  finish_marginal(nx, ad.data(), kd.data(), ad.data() + nx, rq.std_y, rq.std_Z,
                  ate ? rq.Z_x : nullptr, ate ? post.data() : nullptr, rq.map, rq.ci, rq.var,
                  rq.avg);
}

// The grouped pass after the marginal pipeline (ace_model_predict_marginal_groups,
// ace_model_robust_treatment): gcov = E^T (Km_xx - Km_xX A^-1 Km_xX^T) E for
// the indicator E of `label`; prepare (optional) runs after map / ci / var
// are final and before the labels are read.
struct GroupReq {
  int G = 0;
  const int32_t *label = nullptr;
  double *gcov = nullptr;
  std::function<void()> prepare;
};

// The chunk of K_xX the pipeline assembled last (rows c0 .. c0 + nc at K):
// still in the scratch when the pipeline kept it.
struct KeptChunk {
  int64_t c0 = -1, nc = 0;
  const double *K = nullptr;
};

void group_pass(const PredFront &f, const PredOps &op, int64_t nx, const GroupReq &grp,
                KeptChunk kept, PredScratch &ps) {
  ace_model *m = f.m;
  ace_ctx *ctx = m->ctx;
  hipStream_t st = ctx->stream;
  const Shape &s = m->s;
  const int64_t n = m->n;
  const int G = grp.G;
  // S = Km_xX^T E (n x G), chunk by chunk from the last one down: that one is
  // still in the scratch when the pipeline kept it (a new scratch holds no
  // buffer, so it never matches), the others are assembled again; the order
  // does not depend on which, so neither do the sums
  const int64_t chunk = std::min<int64_t>(NXC, nx);
  DBuf dlab, dE, dS, dU, dtmp, dwork, dpart, dR, dQ;
  alloc(ctx, dlab, (size_t)nx * sizeof(int32_t), "alloc labels");
  upload_bytes(ctx, dlab.p, grp.label, (size_t)nx * sizeof(int32_t), "upload labels");
  alloc(ctx, dE, (size_t)(nx * G) * sizeof(double), "alloc E");
  ck(ctx, launch_label_matrix(dlab.i(), nx, G, dE.d(), st), "label matrix");
  alloc(ctx, dS, (size_t)(n * G) * sizeof(double), "alloc S");
  alloc(ctx, dU, (size_t)(n * G) * sizeof(double), "alloc U");
  alloc(ctx, dQ, (size_t)(2 * G * G) * sizeof(double), "alloc Q");
  const int64_t nwork = std::max(gemm_tn_work(n, G, chunk),
                                 std::max(gemm_tn_work(G, G, nx), gemm_tn_work(G, G, n)));
  alloc(ctx, dwork, (size_t)nwork * sizeof(double), "alloc gemm partials");
  bool first = true;
  for (int64_t c0 = (nx - 1) / chunk * chunk; c0 >= 0; c0 -= chunk) {
    const int64_t nc = std::min<int64_t>(chunk, nx - c0);
    int64_t ldk = nc;
    const double *Kc = (kept.K && kept.K == ps.K.d() && kept.c0 == c0 && kept.nc == nc)
                           ? kept.K
                           : op.cross(c0, nc, &ldk, ps.K);
    ck(ctx, launch_gemm_tn(n, G, nc, Kc, ldk, dE.d() + c0, nx, dS.d(), n, !first, dwork.d(), st),
       "S += K^T E");
    first = false;
    kept.K = nullptr;  // only the first chunk of this loop can be the kept one
  }
  // U = A^-1 S (this rank's share when sharded), Q_inv = S^T U
  symm_resident(m, dS.d(), n, false, G, dU.d(), dtmp);
  double *Qinv = dQ.d(), *Qxx = dQ.d() + G * G;
  ck(ctx, launch_gemm_tn(G, G, n, dS.d(), n, dU.d(), n, Qinv, G, false, dwork.d(), st), "S^T U");
  if (m->shard) shard_allreduce_sum(m->shard, Qinv, (int64_t)G * G);
  // R = Km_xx E without Km_xx, Q_xx = E^T R
  alloc(ctx, dpart, (size_t)(group_sums_parts(nx) * nx * G) * sizeof(double), "alloc R partials");
  alloc(ctx, dR, (size_t)(nx * G) * sizeof(double), "alloc R");
  ck(ctx, launch_group_sums(s.kind, s.PM, f.test.view(nx), s.B, s.ZS, f.tv, f.b0, f.b1, dlab.i(), G,
                            dpart.d(), dR.d(), st),
     "grouped kernel sums");
  ck(ctx, launch_gemm_tn(G, G, nx, dE.d(), nx, dR.d(), nx, Qxx, G, false, dwork.d(), st), "E^T R");
  std::vector<double> q((size_t)(2 * G * G));
  download(ctx, q.data(), dQ.d(), q.size(), "download group sums");
  sync(ctx);
  for (int e = 0; e < G * G; ++e) grp.gcov[e] = q[(size_t)(G * G + e)] - q[(size_t)e];
}

// ace_model_predict (rq.marginal = false) / ace_model_predict_marginal: the
// model's resident inverse, K_xX assembled from the resident training side;
// rq's sigma and mu come from theta.  grp: the grouped pass after it.
void predict_impl(ace_model *m, const double *theta, const double *X2, const double *Zt,
                  PredReq rq, const GroupReq *grp = nullptr) {
  ace_ctx *ctx = m->ctx;
  hipStream_t st = ctx->stream;
  const Shape &s = m->s;
  const int64_t n = m->n, nx = rq.nx;
  rq.sigma = theta[0];
  rq.mu = theta[1];
  const PredFront f(m, theta, nx, X2, Zt, rq.marginal, FRONT_W | FRONT_TRI);
  PredOps op;
  op.ctx = ctx;
  op.n = n;
  op.w = f.dw.d();
  op.symm = [&](const double *V, int64_t ldv, int64_t k, double *out, DBuf &tmp) {
    symm_resident(m, V, ldv, true, k, out, tmp);
  };
  if (f.tri) {  // -A^-1 is stored: scale -1
    op.sdiag = f.ddiag.d();
    op.trmm = [&](const double *V, int64_t ldv, int64_t k, double *out) {
      ck(ctx, launch_trmm_lower(m->sw.A.d(), m->naug, n, V, ldv, k, -1.0, out, n, st), "trmm");
    };
    op.symv = [&](const double *V, int64_t ldv, int64_t k, double *out, DBuf &tmp) {
      symm_resident(m, V, ldv, false, k, out, tmp);
    };
    op.ainv_w = [&](double *dst) { f.ainv_w(dst); };
  }
  if (m->shard) op.allreduce = [&](double *b, int64_t c) { shard_allreduce_sum(m->shard, b, c); };
  KeptChunk kept;
  op.cross = [&](int64_t c0, int64_t nc, int64_t *ld, DBuf &scratch) -> const double * {
    alloc(ctx, scratch, (size_t)(nc * n) * sizeof(double), "alloc K_xX");
    kept.c0 = c0;
    kept.nc = nc;
    kept.K = scratch.d();
    // kernmat_*_cpp(X2, X, Z2, Z): test side first
    ck(ctx, launch_assembly(2, s.kind, s.PM, chunk_view(f.test, s, c0, nc), f.train, s.B, s.ZS,
                            f.tv, scratch.d(), nc, nullptr, st, f.b0, f.b1),
       "cross assembly");
    *ld = nc;
    return scratch.d();
  };
  op.kdiag = [&](double *dst) {
    ck(ctx, launch_kdiag(s.kind, f.test.view(nx), s.ZS, f.tv, f.b0, f.b1, dst, st),
       "kernel diagonal");
  };
  op.kxx = [&](int64_t *ld, DBuf &scratch) -> const double * {
    alloc(ctx, scratch, (size_t)(nx * nx) * sizeof(double), "alloc K_xx");
    ck(ctx, launch_assembly(1, s.kind, s.PM, f.test.view(nx), f.test.view(nx), s.B, s.ZS, f.tv,
                            scratch.d(), nx, nullptr, st, f.b0, f.b1),
       "symmetric assembly");
    *ld = nx;
    return scratch.d();
  };
  pred_pipeline(op, rq);
  if (!grp) return;
  if (grp->prepare) grp->prepare();
  // (gcov is written only at the pass's end; a second run starts from what
  // the pipeline left, which a new scratch never matches)
  const KeptChunk after_pipeline = kept;
  with_pred_scratch(ctx, [&](PredScratch &ps) { group_pass(f, op, nx, *grp, after_pipeline, ps); });
}

// ACE_COEF_CHUNK: test points per chunk of the coefficient pass (default and
// upper limit NXC / B: the scratch of an NXC-point prediction chunk)
int64_t coef_chunk(int B) {
  static const int v = env_int("ACE_COEF_CHUNK", 0);
  const int64_t hi = NXC / B;
  return v < 1 ? hi : std::min<int64_t>(v, hi);
}

// Kc ((tc.n B) x n, ld tc.n B): slice b of the chunk's test point c in row
// c + tc.n b.  k_cross_slices_mm does not read tc's basis.
void slice_assembly(ace_ctx *ctx, const Shape &s, PairSide tc, PairSide train, TabView tv,
                    double *Kc) {
  ck(ctx, launch_cross_slices_mm(s.kind, s.PM, tc, train, s.B, s.ZS, tv, Kc, tc.n * s.B,
                                 ctx->stream),
     "slice assembly");
}

// ace_model_coef_cross: the cube Kc (nx x n x B), chunked like the pass; it
// needs neither w nor an inverse
void coef_cross(ace_model *m, const double *theta, int64_t nx, const double *X2, double *out) {
  ace_ctx *ctx = m->ctx;
  const Shape &s = m->s;
  const int64_t n = m->n;
  const int B = s.B;
  const PredFront f(m, theta, nx, X2, nullptr, false, 0);
  DBuf dK;
  const int64_t chunk = std::min<int64_t>(coef_chunk(B), nx);
  alloc(ctx, dK, (size_t)(chunk * B * n) * sizeof(double), "alloc Kc");
  std::vector<double> h((size_t)(chunk * B * n));
  for (int64_t c0 = 0; c0 < nx; c0 += chunk) {
    const int64_t nc = std::min<int64_t>(chunk, nx - c0), ldk = nc * B;
    slice_assembly(ctx, s, chunk_view(f.test, s, c0, nc), f.train, f.tv, dK.d());
    download(ctx, h.data(), dK.d(), (size_t)(ldk * n), "download Kc");
    sync(ctx);
    // (q: the device's training point, the caller's perm[q] when the model
    // holds its points in the zero-pattern order)
    for (int b = 0; b < B; ++b)
      for (int64_t q = 0; q < n; ++q) {
        const int64_t qo = m->perm.empty() ? q : m->perm[(size_t)q];
        for (int64_t c = 0; c < nc; ++c)
          out[c0 + c + nx * (qo + n * b)] = h[(size_t)(c + nc * b + q * ldk)];
      }
  }
}

// ace_model_coef_posterior: m_c = Kc_c A^-1 (y - mu) into mean (nx x B) and
// P_c = Kc_c A^-1 Kc_c^T into P (nx x B x B), Kc_c the B per-slice cross
// kernels of point c without a test basis factor.  Per chunk of ncx points:
// the slices as an (ncx B) x n matrix (k_cross_slices_mm), its product with
// the inverse as predict_impl takes it (strictly lower triangle on one GPU,
// the full symmetric product otherwise), and the B x B Gram sums per point
// (k_coef_gram).  Outputs are written only at the end.
void coef_pass(ace_model *m, const double *theta, int64_t nx, const double *X2, double *mean,
               double *P, PredScratch &ps) {
  ace_ctx *ctx = m->ctx;
  hipStream_t st = ctx->stream;
  const Shape &s = m->s;
  const int64_t n = m->n;
  const int B = s.B;
  const PredFront f(m, theta, nx, X2, nullptr, false, FRONT_W | FRONT_TRI);
  DBuf dsv, dtmp, dpart, dres;
  if (f.tri) {
    alloc(ctx, dsv, (size_t)n * sizeof(double), "alloc s");
    f.ainv_w(dsv.d());
  }
  const int64_t chunk = std::min<int64_t>(coef_chunk(B), nx);
  const int64_t per = (int64_t)B * (B + 1);  // results per point
  alloc(ctx, ps.K, (size_t)(chunk * B * n) * sizeof(double), "alloc Kc");
  alloc(ctx, ps.T, (size_t)(chunk * B * n) * sizeof(double), "alloc T");
  alloc(ctx, dpart, (size_t)coef_gram_work(n, chunk, B) * sizeof(double), "alloc Gram partials");
  alloc(ctx, dres, (size_t)(nx * per) * sizeof(double), "alloc Gram sums");
  for (int64_t c0 = 0; c0 < nx; c0 += chunk) {
    const int64_t nc = std::min<int64_t>(chunk, nx - c0), ldk = nc * B;
    double *Kc = ps.K.d(), *T = ps.T.d(), *res = dres.d() + c0 * per;
    slice_assembly(ctx, s, chunk_view(f.test, s, c0, nc), f.train, f.tv, Kc);
    if (f.tri) {
      ck(ctx, launch_trmm_lower(m->sw.A.d(), m->naug, n, Kc, ldk, ldk, -1.0, T, n, st), "trmm");
      ck(ctx, launch_coef_gram(true, Kc, ldk, T, n, n, nc, B, dsv.d(), f.ddiag.d(), dpart.d(), res,
                               st),
         "coefficient Gram");
    } else {
      symm_resident(m, Kc, ldk, true, ldk, T, dtmp);
      ck(ctx, launch_coef_gram(false, Kc, ldk, T, n, n, nc, B, f.dw.d(), nullptr, dpart.d(), res,
                               st),
         "coefficient Gram");
      if (m->shard) shard_allreduce_sum(m->shard, res, nc * per);
    }
  }
  std::vector<double> h((size_t)(nx * per));
  download(ctx, h.data(), dres.d(), h.size(), "download Gram sums");
  sync(ctx);
  for (int64_t c0 = 0; c0 < nx; c0 += chunk) {
    const int64_t nc = std::min<int64_t>(chunk, nx - c0);
    const double *r = h.data() + c0 * per;
    for (int64_t e = 0; e < nc * B * B; ++e) P[c0 + e % nc + nx * (e / nc)] = r[e];
    for (int64_t e = 0; e < nc * B; ++e) mean[c0 + e % nc + nx * (e / nc)] = r[nc * B * B + e];
  }
}

// cov_c = diag(exp(lambda_b)) - P_c in place: the prior of g(x_c) is
// diagonal, k_b(x, x) = exp(lambda_b), lambda_b = theta[2 + b] (make_tab)
void coef_cov_from_gram(const double *theta, int64_t nx, int B, double *cov) {
  for (int b2 = 0; b2 < B; ++b2)
    for (int b = 0; b < B; ++b) {
      double *e = cov + nx * (b + (int64_t)B * b2);
      const double prior = b == b2 ? std::exp(theta[2 + b]) : 0.0;
      for (int64_t c = 0; c < nx; ++c) e[c] = prior - e[c];
    }
}

// mean (nx x B) and cov (nx x B x B) of the coefficient functions
void coef_posterior(ace_model *m, const double *theta, int64_t nx, const double *X2, double *mean,
                    double *cov) {
  with_pred_scratch(m->ctx,
                    [&](PredScratch &ps) { coef_pass(m, theta, nx, X2, mean, cov, ps); });
  coef_cov_from_gram(theta, nx, m->s.B, cov);
}

// ace_model_coef_groups: the posterior of the summed coefficient vectors
// sum_{c in g} g(x_c) of the G groups of `label`, modelled on group_pass.
// With s_{g,b} = sum_{c in g} Kc_b(x_c, X)^T (n-vectors, the columns of S):
//   gmean[g,b]         = s_{g,b}^T A^-1 (y - mu)
//   gcov[(g,b),(h,b')] = delta_bb' sum_{c in g, c' in h} k_b(x_c, x_c')
//                        - s_{g,b}^T A^-1 s_{h,b'}.
// S (n x G B) comes from k_group_slices_mm with the training side as rows --
// the (nx B) x n matrix Kc is never formed, so the test points are not
// chunked -- U = A^-1 S is G B right-hand sides (the rank's share when
// sharded, then one all-reduce of G B (G B + 1) doubles), and the prior term
// is the same kernel on the test points against themselves, then E^T R' (one
// G x G block per slice).  The training rows are in the device's order, which
// no output shows.  gcov is symmetrised exactly on the host; outputs are
// written only at the end.
void coef_group_pass(ace_model *m, const double *theta, int64_t nx, const double *X2, int G,
                     const int32_t *label, double *gmean, double *gcov, int64_t *gcount,
                     PredScratch &ps) {
  ace_ctx *ctx = m->ctx;
  hipStream_t st = ctx->stream;
  const Shape &s = m->s;
  const int64_t n = m->n;
  const int B = s.B;
  const int64_t GB = (int64_t)G * B;
  const PredFront f(m, theta, nx, X2, nullptr, false, FRONT_W);
  const PairSide tp = f.test.view(nx);
  DBuf dlab, dE, dpart, dR, dQ, dwork, dtmp;
  alloc(ctx, dlab, (size_t)nx * sizeof(int32_t), "alloc labels");
  upload_bytes(ctx, dlab.p, label, (size_t)nx * sizeof(int32_t), "upload labels");
  alloc(ctx, dE, (size_t)(nx * G) * sizeof(double), "alloc E");
  ck(ctx, launch_label_matrix(dlab.i(), nx, G, dE.d(), st), "label matrix");
  alloc(ctx, ps.K, (size_t)(n * GB) * sizeof(double), "alloc S");
  alloc(ctx, ps.T, (size_t)(n * GB) * sizeof(double), "alloc U");
  const int64_t npart =
      std::max(group_slices_parts(n, nx) * n, group_slices_parts(nx, nx) * nx) * GB;
  alloc(ctx, dpart, (size_t)npart * sizeof(double), "alloc grouped partials");
  double *S = ps.K.d(), *U = ps.T.d();
  ck(ctx, launch_group_slices(s.kind, s.PM, f.train, tp, B, s.ZS, f.tv, dlab.i(), G, dpart.d(), S,
                              st),
     "grouped slice sums (S)");
  symm_resident(m, S, n, false, GB, U, dtmp);
  // [Q_inv (G B x G B) | gmean (G B) | Q_xx (G x G per slice)]
  alloc(ctx, dQ, (size_t)(GB * (GB + 1) + (int64_t)G * GB) * sizeof(double), "alloc Q");
  double *Qinv = dQ.d(), *gm = Qinv + GB * GB, *Qxx = gm + GB;
  const int64_t nwork = std::max(gemm_tn_work(GB, GB, n),
                                 std::max(gemm_tn_work(GB, 1, n), gemm_tn_work(G, GB, nx)));
  alloc(ctx, dwork, (size_t)nwork * sizeof(double), "alloc gemm partials");
  ck(ctx, launch_gemm_tn(GB, GB, n, S, n, U, n, Qinv, GB, false, dwork.d(), st), "S^T U");
  ck(ctx, launch_gemm_tn(GB, 1, n, U, n, f.dw.d(), n, gm, GB, false, dwork.d(), st), "U^T w");
  if (m->shard) shard_allreduce_sum(m->shard, Qinv, GB * (GB + 1));
  // R' = K_b(x, x) E per slice without K_b, Q_xx,b = E^T R'_b
  alloc(ctx, dR, (size_t)(nx * GB) * sizeof(double), "alloc R");
  ck(ctx, launch_group_slices(s.kind, s.PM, tp, tp, B, s.ZS, f.tv, dlab.i(), G, dpart.d(), dR.d(),
                              st),
     "grouped slice sums (prior)");
  ck(ctx, launch_gemm_tn(G, GB, nx, dE.d(), nx, dR.d(), nx, Qxx, G, false, dwork.d(), st), "E^T R");
  std::vector<double> q((size_t)(GB * (GB + 1) + (int64_t)G * GB));
  download(ctx, q.data(), dQ.d(), q.size(), "download group sums");
  sync(ctx);
  const double *hQinv = q.data(), *hgm = hQinv + GB * GB, *hQxx = hgm + GB;
  // index i = g + G b; the prior of g_b is independent across b
  const auto raw = [&](int64_t i, int64_t j) {
    const int64_t b = i / G, b2 = j / G;
    const double prior = b == b2 ? hQxx[i % G + (int64_t)G * (j % G + (int64_t)G * b)] : 0.0;
    return prior - hQinv[i + GB * j];
  };
  for (int64_t j = 0; j < GB; ++j)
    for (int64_t i = 0; i < GB; ++i) gcov[i + GB * j] = 0.5 * (raw(i, j) + raw(j, i));
  std::copy(hgm, hgm + GB, gmean);
  std::fill(gcount, gcount + G, (int64_t)0);
  for (int64_t c = 0; c < nx; ++c)
    if (label[c] >= 0) ++gcount[label[c]];
}

// the arguments ace_model_coef_groups and ace_model_average_response share
void coef_group_args(ace_model *m, int64_t nx, int G, const int32_t *label) {
  ace_ctx *ctx = m->ctx;
  arg(ctx, G >= 1 && G <= 64, "G must be in [1, 64]");
  arg(ctx, (int64_t)G * m->s.B <= 2048, "G * B must be <= 2048");
  for (int64_t i = 0; i < nx; ++i)
    arg(ctx, label[i] >= -1 && label[i] < G, "label outside [-1, G)");
}

// ace_model_predict_joint: the joint posterior at nx <= JOINT_NX test points
// of a single-GPU model.  K_xX, T' = A^-1 K_xX^T (the full symmetric product:
// the triangular form only serves the diagonal) and K_xx as predict_impl
// builds them, in the retained scratch; then C = scale (K_xx - K_xX T' +
// noise I) (k_post_cov), its factor L (launch_potrf_lower, no host sync
// between the steps) and D = m 1^T + L xi.  C, L and the draws are scratch of
// this call alone (PredScratch holds what the other calls share).  The
// factor's flag is read once, with the results; outputs are written only at
// the end.
constexpr int64_t JOINT_NX = 8192, JOINT_S = 4096;

struct JointReq {
  bool marginal = false, noise = false;
  double mean_y = 0.0, std_y = 1.0, std_Z = 1.0, jitter = 0.0;
  int64_t S = 0;
  const double *xi = nullptr;
  double *map = nullptr, *cov = nullptr, *L = nullptr, *draws = nullptr;
  int64_t *info = nullptr;
};

void joint_pass(ace_model *m, const double *theta, int64_t nx, const double *X2, const double *Zt,
                const JointReq &rq, PredScratch &ps) {
  ace_ctx *ctx = m->ctx;
  hipStream_t st = ctx->stream;
  const Shape &s = m->s;
  const int64_t n = m->n;
  const int B = s.B;
  const bool marginal = rq.marginal;
  const double mu = theta[1];
  const bool factor = rq.L || rq.S > 0;
  const PredFront f(m, theta, nx, X2, Zt, marginal, FRONT_W);
  DBuf dad, dtmp, dC, dL, dxi, dD, dmap, dflag;
  alloc(ctx, ps.K, (size_t)(nx * n) * sizeof(double), "alloc K_xX");
  alloc(ctx, ps.T, (size_t)(nx * n) * sizeof(double), "alloc T");
  alloc(ctx, ps.Kxx, (size_t)(nx * nx) * sizeof(double), "alloc K_xx");
  alloc(ctx, dC, (size_t)(nx * nx) * sizeof(double), "alloc C");
  alloc(ctx, dad, (size_t)(2 * nx) * sizeof(double), "alloc sums");
  // kernmat_*_cpp(X2, X, Z2, Z): test side first
  ck(ctx, launch_assembly(2, s.kind, s.PM, f.test.view(nx), f.train, B, s.ZS, f.tv, ps.K.d(), nx,
                          nullptr, st, f.b0, f.b1),
     "cross assembly");
  symm_resident(m, ps.K.d(), nx, true, nx, ps.T.d(), dtmp);
  ck(ctx, launch_pred_cols(ps.T.d(), n, ps.K.d(), nx, n, nx, f.dw.d(), dad.d(), dad.d() + nx, st),
     "pred sums");
  ck(ctx, launch_assembly(1, s.kind, s.PM, f.test.view(nx), f.test.view(nx), B, s.ZS, f.tv,
                          ps.Kxx.d(), nx, nullptr, st, f.b0, f.b1),
     "symmetric assembly");
  const double sc = marginal ? rq.std_y / rq.std_Z : rq.std_y;
  const double noise = (!marginal && rq.noise) ? std::exp(theta[0]) : 0.0;
  ck(ctx, launch_post_cov(ps.K.d(), nx, ps.T.d(), n, n, ps.Kxx.d(), nx, nx, noise, sc * sc,
                          dC.d(), nx, st),
     "posterior covariance");
  if (factor) {
    alloc(ctx, dL, (size_t)(nx * nx) * sizeof(double), "alloc L");
    alloc(ctx, dflag, sizeof(int), "alloc flag");
    ck(ctx, launch_potrf_lower(dC.d(), nx, nx, rq.jitter, dL.d(), nx, dflag.i(), st), "factor");
  }
  // the map needs the sums on the host (finish_pred / finish_marginal state it)
  std::vector<double> ad((size_t)(2 * nx)), zero((size_t)nx, 0.0), hmap((size_t)nx),
      hci((size_t)(2 * nx)), hvar((size_t)nx);
  download(ctx, ad.data(), dad.d(), ad.size(), "download sums");
  sync(ctx);
  if (!marginal)
    finish_pred(nx, ad.data(), zero.data(), zero.data(), theta[0], mu, rq.mean_y, rq.std_y,
                hmap.data(), hci.data(), hvar.data());
  else
    finish_marginal(nx, ad.data(), zero.data(), zero.data(), rq.std_y, rq.std_Z, nullptr, nullptr,
                    hmap.data(), hci.data(), hvar.data(), nullptr);
  if (rq.S > 0) {
    upload(ctx, dmap, hmap.data(), hmap.size(), "upload map");
    upload(ctx, dxi, rq.xi, (size_t)(nx * rq.S), "upload xi");
    alloc(ctx, dD, (size_t)(nx * rq.S) * sizeof(double), "alloc draws");
    ck(ctx, launch_draws(dL.d(), nx, nx, dxi.d(), rq.S, dmap.d(), dD.d(), st), "draws");
  }
  int flag = 0;
  if (factor) {
    sync(ctx);
    ck(ctx, hipMemcpyAsync(&flag, dflag.p, sizeof(int), hipMemcpyDeviceToHost, st), "download flag");
    sync(ctx);
  }
  if (rq.cov) download(ctx, rq.cov, dC.d(), (size_t)(nx * nx), "download cov");
  if (flag == 0) {
    if (rq.L) download(ctx, rq.L, dL.d(), (size_t)(nx * nx), "download L");
    if (rq.S > 0) download(ctx, rq.draws, dD.d(), (size_t)(nx * rq.S), "download draws");
  }
  sync(ctx);
  if (flag != 0) {  // a numerical outcome: map and cov stay valid
    if (rq.L) std::fill(rq.L, rq.L + nx * nx, kNaN);
    if (rq.S > 0) std::fill(rq.draws, rq.draws + nx * rq.S, kNaN);
  }
  std::copy(hmap.begin(), hmap.end(), rq.map);
  *rq.info = flag;
}

void unsupported(ace_ctx *ctx, bool ok, const char *msg) {
  if (ok) return;
  ctx->err = msg;
  throw Fail{ACE_ERR_UNSUPPORTED};
}

// gsum / gcount of ace_model_predict_marginal_groups from the final map
void group_sums_host(int64_t nx, int G, const int32_t *label, const double *map, double *gsum,
                     int64_t *gcount) {
  for (int g = 0; g < G; ++g) {
    gsum[g] = 0.0;
    gcount[g] = 0;
  }
  for (int64_t i = 0; i < nx; ++i)
    if (label[i] >= 0) {
      gsum[label[i]] += map[i];
      ++gcount[label[i]];
    }
}

// Every ace_model_* entry point below, in this order: the device, the
// arguments all of them need (ok), the entry point's own checks (more), then
// the model's state -- data, and a resident inverse unless need_inverse is off.
void enter(ace_model *m, bool ok, const std::function<void()> &more = {},
           bool need_inverse = true) {
  ace_ctx *ctx = m->ctx;
  ck(ctx, hipSetDevice(ctx->device), "hipSetDevice");
  arg(ctx, ok, "bad shape / null argument");
  if (more) more();
  arg(ctx, m->has_data, "ace_model_set_data() not called");
  if (need_inverse)
    arg(ctx, m->has_inverse, "no resident inverse: call ace_model_para_update() first");
}

// the arguments of the four pipeline entry points
bool pred_args(const ace_model *m, int64_t nx, const double *theta, const double *X2,
               const double *Z2, const double *map, const double *ci, const double *var) {
  return nx >= 1 && theta && map && ci && var && (m->s.p == 0 || X2) && (m->s.B == 1 || Z2);
}

PredReq marginal_req(int64_t nx, double std_y, double std_Z, double *map, double *ci, double *var) {
  PredReq rq(nx, std_y, map, ci, var);
  rq.marginal = true;
  rq.std_Z = std_Z;
  return rq;
}

}  // namespace

// The device prediction pipeline (pred_cpp / pred_marginal_cpp semantics)
// over abstract operands -- the device model's resident inverse here, and the
// device-matrix handles of the R6-faithful path in ace_dmat.cpp -- in the
// context's retained scratch (with_pred_scratch).
void pred_pipeline(const PredOps &op, const PredReq &rq) {
  with_pred_scratch(op.ctx, [&](PredScratch &ps) { pipeline_body(op, rq, ps); });
}

extern "C" {

int ace_model_apply_inverse(ace_model *m, int64_t k, const double *V, double *out) {
  if (!m) return ACE_ERR_ARG;
  ace_ctx *ctx = m->ctx;
  ACE_TRY
  enter(m, k >= 1 && V && out);
  const int64_t n = m->n;
  DBuf dV, dout, dtmp;
  // a model that holds its points in the zero-pattern order (ace_model::perm):
  // V's rows go in, and the result's rows come back, through that order
  const std::vector<int64_t> &perm = m->perm;
  std::vector<double> hp;
  if (!perm.empty()) {
    hp.resize((size_t)(n * k));
    for (int64_t c = 0; c < k; ++c)
      for (int64_t q = 0; q < n; ++q) hp[(size_t)(q + c * n)] = V[perm[(size_t)q] + c * n];
  }
  upload(ctx, dV, perm.empty() ? V : hp.data(), (size_t)(n * k), "upload V");
  alloc(ctx, dout, (size_t)(n * k) * sizeof(double), "alloc out");
  symm_resident(m, dV.d(), n, false, k, dout.d(), dtmp);
  if (m->shard) shard_allreduce_sum(m->shard, dout.d(), n * k);
  download(ctx, perm.empty() ? out : hp.data(), dout.d(), (size_t)(n * k), "download out");
  sync(ctx);
  if (!perm.empty())
    for (int64_t c = 0; c < k; ++c)
      for (int64_t q = 0; q < n; ++q) out[perm[(size_t)q] + c * n] = hp[(size_t)(q + c * n)];
  return ACE_OK;
  ACE_CATCH
}

int ace_model_predict(ace_model *m, const double *theta, int64_t nx, const double *X2,
                      const double *Z2, double mean_y, double std_y, double *map, double *ci,
                      double *var) {
  if (!m) return ACE_ERR_ARG;
  ace_ctx *ctx = m->ctx;
  ACE_TRY
  enter(m, pred_args(m, nx, theta, X2, Z2, map, ci, var));
  PredReq rq(nx, std_y, map, ci, var);
  rq.mean_y = mean_y;
  predict_impl(m, theta, X2, Z2, rq);
  return ACE_OK;
  ACE_CATCH
}

int ace_model_predict_marginal(ace_model *m, const double *theta, int64_t nx, const double *X2,
                               const double *dZ2, const double *Z_x, double std_y, double std_Z,
                               int calculate_ate, double *map, double *ci, double *var,
                               double *avg) {
  if (!m) return ACE_ERR_ARG;
  ace_ctx *ctx = m->ctx;
  ACE_TRY
  enter(m, pred_args(m, nx, theta, X2, dZ2, map, ci, var), [&] {
    arg(ctx, !calculate_ate || (Z_x && avg), "calculate_ate needs Z_x and avg");
  });
  PredReq rq = marginal_req(nx, std_y, std_Z, map, ci, var);
  rq.Z_x = Z_x;
  rq.ate = calculate_ate;
  rq.avg = avg;
  predict_impl(m, theta, X2, dZ2, rq);
  return ACE_OK;
  ACE_CATCH
}

int ace_model_predict_marginal_groups(ace_model *m, const double *theta, int64_t nx,
                                      const double *X2, const double *dZ2, double std_y,
                                      double std_Z, int G, const int32_t *label, double *map,
                                      double *ci, double *var, double *gsum, int64_t *gcount,
                                      double *gcov) {
  if (!m) return ACE_ERR_ARG;
  ace_ctx *ctx = m->ctx;
  ACE_TRY
  enter(m, pred_args(m, nx, theta, X2, dZ2, map, ci, var), [&] {
    arg(ctx, label && gsum && gcount && gcov, "null argument");
    arg(ctx, G >= 1 && G <= 64, "G must be in [1, 64]");
    for (int64_t i = 0; i < nx; ++i)
      arg(ctx, label[i] >= -1 && label[i] < G, "label outside [-1, G)");
  });
  const GroupReq grp{G, label, gcov, nullptr};
  predict_impl(m, theta, X2, dZ2, marginal_req(nx, std_y, std_Z, map, ci, var), &grp);
  group_sums_host(nx, G, label, map, gsum, gcount);
  return ACE_OK;
  ACE_CATCH
}

int ace_model_robust_treatment(ace_model *m, const double *theta, int64_t nx, const double *X2,
                               const double *dZ2, const double *Z_x, double std_y, double std_Z,
                               int n_steps, double *map, double *ci, double *var,
                               double *thresholds, int32_t *level, double *avg, int64_t *counts) {
  if (!m) return ACE_ERR_ARG;
  ace_ctx *ctx = m->ctx;
  ACE_TRY
  enter(m, pred_args(m, nx, theta, X2, dZ2, map, ci, var), [&] {
    arg(ctx, Z_x && thresholds && level && avg && counts, "null argument");
    arg(ctx, n_steps >= 1 && n_steps <= 31, "n_steps must be in [1, 31]");
    for (int64_t i = 0; i < nx; ++i)
      arg(ctx, Z_x[i] == 0.0 || Z_x[i] == 1.0, "Z_x must be 0 or 1 (binary treatment)");
  });
  const int T = n_steps + 1, G = 2 * T;
  std::vector<int32_t> label((size_t)nx);
  std::vector<double> gcov((size_t)(G * G));
  GroupReq grp{G, label.data(), gcov.data(), nullptr};
  grp.prepare = [&]() {
    const int st = ace_robust_levels(nx, var, n_steps, thresholds, level);
    if (st != ACE_OK) {
      ctx->err = "robust_treatment: non-finite posterior variance";
      throw Fail{st};
    }
    for (int64_t i = 0; i < nx; ++i) label[(size_t)i] = 2 * level[i] + (Z_x[i] == 1.0 ? 1 : 0);
  };
  predict_impl(m, theta, X2, dZ2, marginal_req(nx, std_y, std_Z, map, ci, var), &grp);
  std::vector<double> gsum((size_t)G);
  std::vector<int64_t> gcount((size_t)G);
  group_sums_host(nx, G, label.data(), map, gsum.data(), gcount.data());
  // step t keeps the groups of levels <= t: prefix sums of gsum, gcount, gcov
  for (int t = 0; t < T; ++t) {
    const int g1 = 2 * (t + 1);
    double sy = 0.0, syz = 0.0, post[3] = {0.0, 0.0, 0.0};
    int64_t kept = 0, treated = 0;
    for (int g = 0; g < g1; ++g) {
      sy += gsum[(size_t)g];
      kept += gcount[(size_t)g];
      if (g & 1) {
        syz += gsum[(size_t)g];
        treated += gcount[(size_t)g];
      }
    }
    for (int h = 0; h < g1; ++h)
      for (int g = 0; g < g1; ++g) {
        const double c = gcov[(size_t)(g + h * G)];
        post[0] += c;
        if ((g & 1) && (h & 1)) post[1] += c;
        if (!(g & 1) && !(h & 1)) post[2] += c;
      }
    marginal_averages(kept, std_y, sy, syz, (double)treated, post, avg + 12 * t);
    counts[3 * t + 0] = kept;
    counts[3 * t + 1] = treated;
    counts[3 * t + 2] = kept - treated;
  }
  return ACE_OK;
  ACE_CATCH
}

int ace_model_coef_posterior(ace_model *m, const double *theta, int64_t nx, const double *X2,
                             double *mean, double *cov) {
  if (!m) return ACE_ERR_ARG;
  ace_ctx *ctx = m->ctx;
  ACE_TRY
  enter(m, nx >= 1 && theta && mean && cov && (m->s.p == 0 || X2));
  coef_posterior(m, theta, nx, X2, mean, cov);
  return ACE_OK;
  ACE_CATCH
}

int ace_model_coef_cross(ace_model *m, const double *theta, int64_t nx, const double *X2,
                         double *Kc) {
  if (!m) return ACE_ERR_ARG;
  ace_ctx *ctx = m->ctx;
  ACE_TRY
  enter(m, nx >= 1 && theta && Kc && (m->s.p == 0 || X2), {}, false);
  coef_cross(m, theta, nx, X2, Kc);
  return ACE_OK;
  ACE_CATCH
}

int ace_model_predict_surface(ace_model *m, const double *theta, int64_t nx, const double *X2,
                              int64_t nz, const double *Zb, int marginal, double mean_y,
                              double std_y, double std_Z, double *map, double *ci, double *var) {
  if (!m) return ACE_ERR_ARG;
  ace_ctx *ctx = m->ctx;
  ACE_TRY
  const int B = m->s.B;
  enter(m, nx >= 1 && nz >= 1 && theta && map && ci && var && (m->s.p == 0 || X2) && (B == 1 || Zb));
  std::vector<double> mean((size_t)(nx * B)), cov((size_t)(nx * B * B));
  coef_posterior(m, theta, nx, X2, mean.data(), cov.data());
  // beta = (1, B(z)); marginal: (0, dB(z)), (1) for B == 1 (src/pred_cpp.cpp:55-67)
  std::vector<double> W((size_t)(nz * B));
  for (int64_t j = 0; j < nz; ++j) {
    W[(size_t)j] = (marginal && B > 1) ? 0.0 : 1.0;
    for (int b = 1; b < B; ++b) W[(size_t)(j + nz * b)] = Zb[j + nz * (b - 1)];
  }
  const int rc = marginal ? ace_coef_contract(nx, B, nz, mean.data(), cov.data(), W.data(), 0.0,
                                              std_y / std_Z, 0.0, 0.0, map, ci, var)
                          : ace_coef_contract(nx, B, nz, mean.data(), cov.data(), W.data(), mean_y,
                                              std_y, theta[1], std::exp(theta[0]), map, ci, var);
  if (rc != ACE_OK) throw Fail{rc};
  return ACE_OK;
  ACE_CATCH
}

int ace_model_coef_groups(ace_model *m, const double *theta, int64_t nx, const double *X2, int G,
                          const int32_t *label, double *gmean, double *gcov, int64_t *gcount) {
  if (!m) return ACE_ERR_ARG;
  ace_ctx *ctx = m->ctx;
  ACE_TRY
  enter(m, nx >= 1 && theta && label && gmean && gcov && gcount && (m->s.p == 0 || X2),
        [&] { coef_group_args(m, nx, G, label); });
  with_pred_scratch(ctx, [&](PredScratch &ps) {
    coef_group_pass(m, theta, nx, X2, G, label, gmean, gcov, gcount, ps);
  });
  return ACE_OK;
  ACE_CATCH
}

int ace_model_average_response(ace_model *m, const double *theta, int64_t nx, const double *X2,
                               int G, const int32_t *label, int64_t nz, const double *Zb,
                               int marginal, double mean_y, double std_y, double std_Z,
                               double *map, double *ci, double *var, double *cov) {
  if (!m) return ACE_ERR_ARG;
  ace_ctx *ctx = m->ctx;
  ACE_TRY
  const int B = m->s.B;
  enter(m,
        nx >= 1 && nz >= 1 && theta && label && map && ci && var && (m->s.p == 0 || X2) &&
            (B == 1 || Zb),
        [&] { coef_group_args(m, nx, G, label); });
  const int64_t GB = (int64_t)G * B;
  std::vector<double> gmean((size_t)GB), gcov((size_t)(GB * GB));
  std::vector<int64_t> gcount((size_t)G);
  with_pred_scratch(ctx, [&](PredScratch &ps) {
    coef_group_pass(m, theta, nx, X2, G, label, gmean.data(), gcov.data(), gcount.data(), ps);
  });
  // beta as ace_model_predict_surface's, without its noise term
  std::vector<double> W((size_t)(nz * B));
  for (int64_t j = 0; j < nz; ++j) {
    W[(size_t)j] = (marginal && B > 1) ? 0.0 : 1.0;
    for (int b = 1; b < B; ++b) W[(size_t)(j + nz * b)] = Zb[j + nz * (b - 1)];
  }
  const int rc =
      marginal ? ace_coef_group_contract(G, B, nz, gmean.data(), gcov.data(), gcount.data(),
                                         W.data(), 0.0, std_y / std_Z, 0.0, map, ci, var, cov)
               : ace_coef_group_contract(G, B, nz, gmean.data(), gcov.data(), gcount.data(),
                                         W.data(), mean_y, std_y, theta[1], map, ci, var, cov);
  if (rc != ACE_OK) throw Fail{rc};
  return ACE_OK;
  ACE_CATCH
}

int ace_model_predict_joint(ace_model *m, const double *theta, int64_t nx, const double *X2,
                            const double *Zt, int marginal, double mean_y, double std_y,
                            double std_Z, int noise, double jitter, int64_t S, const double *xi,
                            double *map, double *cov, double *L, double *draws, int64_t *info) {
  if (!m) return ACE_ERR_ARG;
  ace_ctx *ctx = m->ctx;
  ACE_TRY
  enter(m, nx >= 1 && theta && map && info && (m->s.p == 0 || X2) && (m->s.B == 1 || Zt), [&] {
    arg(ctx, S >= 0 && (S == 0 || (xi && draws)), "S > 0 needs xi and draws");
    arg(ctx, jitter >= 0.0 && std::isfinite(jitter), "jitter must be finite and >= 0");
    unsupported(ctx, !m->shard, "predict_joint: sharded models are not supported (single GPU only)");
    unsupported(ctx, nx <= JOINT_NX, "predict_joint: nx <= 8192 (one chunk; C is 512 MB there)");
    unsupported(ctx, S <= JOINT_S, "predict_joint: S <= 4096 draws per call");
  });
  JointReq rq;
  rq.marginal = marginal != 0;
  rq.noise = noise != 0;
  rq.mean_y = marginal ? 0.0 : mean_y;
  rq.std_y = std_y;
  rq.std_Z = std_Z;
  rq.jitter = jitter;
  rq.S = S;
  rq.xi = xi;
  rq.map = map;
  rq.cov = cov;
  rq.L = L;
  rq.draws = draws;
  rq.info = info;
  with_pred_scratch(ctx, [&](PredScratch &ps) { joint_pass(m, theta, nx, X2, Zt, rq, ps); });
  return ACE_OK;
  ACE_CATCH
}

int ace_potrf_lower(int64_t n, const double *A, int64_t lda, double jitter, double *L, int64_t ldl,
                    int64_t *info) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  ace_ctx *ctx = nullptr;
  const int rc = ace_create(dev, &ctx);
  if (rc != ACE_OK) return rc;
  int code = ACE_OK;
  try {
    arg(ctx, n >= 1 && A && L && info && lda >= n && ldl >= n, "bad shape / null argument");
    arg(ctx, jitter >= 0.0 && std::isfinite(jitter), "jitter must be finite and >= 0");
    unsupported(ctx, n <= 4 * JOINT_NX, "potrf_lower: n <= 32768");
    hipStream_t st = ctx->stream;
    std::vector<double> h((size_t)(n * n));
    for (int64_t c = 0; c < n; ++c) std::copy(A + c * lda, A + c * lda + n, h.begin() + c * n);
    DBuf dA, dL, dflag;
    upload(ctx, dA, h.data(), h.size(), "upload A");
    alloc(ctx, dL, (size_t)(n * n) * sizeof(double), "alloc L");
    alloc(ctx, dflag, sizeof(int), "alloc flag");
    ck(ctx, launch_potrf_lower(dA.d(), n, n, jitter, dL.d(), n, dflag.i(), st), "factor");
    int flag = 0;
    sync(ctx);
    ck(ctx, hipMemcpyAsync(&flag, dflag.p, sizeof(int), hipMemcpyDeviceToHost, st), "download flag");
    download(ctx, h.data(), dL.d(), h.size(), "download L");
    sync(ctx);
    for (int64_t c = 0; c < n; ++c)
      for (int64_t r = 0; r < n; ++r) L[r + c * ldl] = flag ? kNaN : h[(size_t)(r + c * n)];
    *info = flag;
  } catch (const Fail &f) {
    code = f.code;
    g_create_err = ctx->err;  // no context outlives the call: ace_last_error(NULL)
  }
  ace_destroy(ctx);
  return code;
}

}  // extern "C"
