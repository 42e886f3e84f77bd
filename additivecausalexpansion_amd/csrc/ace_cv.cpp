// ace_cv.cpp -- cross-validation from a resident inverse: the
// host core over ace_cv.hip's kernels and the two ABI entry points,
// ace_model_cv (the device model's inverse) and ace_cv_from_inverse (host
// buffers).  The plan -- validation, device rows, classes, scratch -- is
// ace_cv_plan.cpp's.
#include <cmath>
#include <map>
#include <memory>
#include <vector>

#include "../../include/ace_hip.h"

#include "ace_common.h"
#include "ace_cv.h"
#include "ace_model.h"

using namespace ace;

namespace {

// ACE_CV_WG_MAX: the largest fold the workgroup kernel takes (default and
// upper limit CV_WG_MAX); read per call, so a test can send the same folds
// through the whole-chip sweep.
int cv_wg_max() { return env_int("ACE_CV_WG_MAX", CV_WG_MAX); }

void refuse(ace_ctx *ctx, bool ok, const char *msg) {
  if (ok) return;
  ctx->err = msg;
  throw Fail{ACE_ERR_UNSUPPORTED};
}

// Per fold: r and v in the caller's order (pl.total), logdet / mahal /
// status per fold.
struct CvHost {
  std::vector<double> r, v, logdet, mahal;
  std::vector<int> status;
};

// S = sgn * P (device, lower triangle read), alpha (device, n).  Every buffer
// and SweepWork below lives for this call only.
void cv_core(ace_ctx *ctx, const double *P, int64_t ldp, double sgn, const double *alpha,
             const CvPlan &pl, CvHost &out) {
  hipStream_t st = ctx->stream;
  const int64_t nf = pl.nf, total = pl.total;
  DBuf drows, ddesc, dr, dv, dld, dmh, dst, dW, daf;
  alloc(ctx, drows, (size_t)total * sizeof(int64_t), "alloc cv rows");
  upload_bytes(ctx, drows.p, pl.rows.data(), (size_t)total * sizeof(int64_t), "upload cv rows");
  alloc(ctx, dr, (size_t)total * sizeof(double), "alloc cv r");
  alloc(ctx, dv, (size_t)total * sizeof(double), "alloc cv v");
  alloc(ctx, dld, (size_t)nf * sizeof(double), "alloc cv logdet");
  alloc(ctx, dmh, (size_t)nf * sizeof(double), "alloc cv mahal");
  alloc(ctx, dst, (size_t)nf * sizeof(int), "alloc cv status");
  const CvSrc src{P, ldp, sgn, alpha, static_cast<const int64_t *>(drows.p)};
  const CvRes res{dr.d(), dv.d(), dld.d(), dmh.d(), dst.i()};

  if (pl.folds[0].cls == CV_LOO) {
    ck(ctx, launch_cv_loo(src, nf, res, st), "cv loo");
  } else {
    // the descriptors: the workgroup folds, then the sweep folds
    std::vector<CvDesc> desc;
    int64_t ldmax = 0;
    for (const int64_t f : pl.wg) {
      const CvFold &c = pl.folds[(size_t)f];
      desc.push_back(CvDesc{c.off, c.m, c.ld, c.scratch, f});
      ldmax = std::max(ldmax, c.ld);
    }
    const int64_t nwg = (int64_t)pl.wg.size();
    for (const int64_t f : pl.sweep) {
      const CvFold &c = pl.folds[(size_t)f];
      desc.push_back(CvDesc{c.off, c.m, round_up(c.m, NB) + AUG, 0, f});
    }
    alloc(ctx, ddesc, desc.size() * sizeof(CvDesc), "alloc cv folds");
    upload_bytes(ctx, ddesc.p, desc.data(), desc.size() * sizeof(CvDesc), "upload cv folds");
    const CvDesc *dd = static_cast<const CvDesc *>(ddesc.p);
    if (nwg > 0) {
      alloc(ctx, dW, (size_t)pl.wg_doubles * sizeof(double), "alloc cv scratch");
      ck(ctx, launch_cv_gather(src, dd, nwg, ldmax, dW.d(), 0, nullptr, st), "cv gather");
      ck(ctx, launch_cv_fold(dd, nwg, pl.wg_mmax, dW.d(), res, st), "cv fold");
    }
    // Large folds, one after another on the whole-chip sweep, as
    // ace_invkernel runs it.  One SweepWork per padded size, ensured once: its
    // counter offsets depend on the step count (ace_model.h).
    std::map<int64_t, std::unique_ptr<SweepWork>> works;
    for (size_t j = 0; j < pl.sweep.size(); ++j) {
      const CvFold &c = pl.folds[(size_t)pl.sweep[j]];
      const int64_t npad = round_up(c.m, NB);
      refuse(ctx, npad + AUG <= 65535, "cv: a fold of more than 65280 rows is not supported");
      std::unique_ptr<SweepWork> &wp = works[npad];
      if (!wp) {
        wp.reset(new SweepWork());
        wp->ensure(ctx, c.m);
      }
      SweepWork &w = *wp;
      alloc(ctx, daf, (size_t)npad * sizeof(double), "alloc cv rhs");
      ck(ctx, launch_cv_gather(src, dd + nwg + j, 1, w.naug, w.A.d(), w.npad, daf.d(), st),
         "cv gather");
      ck(ctx, launch_aug_init(w.A.d(), w.naug, w.npad, c.m, daf.d(), st), "aug init");
      ck(ctx, hipMemsetAsync(w.flag.p, 0, sizeof(int), st), "memset flag");
      const SweepSync sy = w.sync(ctx);
      ck(ctx, run_sweep(w.bufs(), st, &sy, nullptr), "sweep");
      ck(ctx, launch_cv_sweep_out(w.A.d(), w.naug, w.npad, w.piv.d(), w.flag.i(), dd + nwg + j,
                                  res, st),
         "cv sweep out");
    }
    sync(ctx);  // the SweepWorks are freed on return
  }

  std::vector<double> hr((size_t)total), hv((size_t)total);
  out.logdet.resize((size_t)nf);
  out.mahal.resize((size_t)nf);
  out.status.resize((size_t)nf);
  download(ctx, hr.data(), dr.d(), (size_t)total, "download cv r");
  download(ctx, hv.data(), dv.d(), (size_t)total, "download cv v");
  download(ctx, out.logdet.data(), dld.d(), (size_t)nf, "download cv logdet");
  download(ctx, out.mahal.data(), dmh.d(), (size_t)nf, "download cv mahal");
  ck(ctx, hipMemcpyAsync(out.status.data(), dst.p, (size_t)nf * sizeof(int), hipMemcpyDeviceToHost,
                         st),
     "download cv status");
  sync(ctx);
  // back to the caller's order inside each fold
  out.r.resize((size_t)total);
  out.v.resize((size_t)total);
  for (const CvFold &c : pl.folds)
    for (int64_t k = 0; k < c.m; ++k) {
      const size_t to = (size_t)(c.off + pl.scatter[(size_t)(c.off + k)]);
      out.r[to] = hr[(size_t)(c.off + k)];
      out.v[to] = hv[(size_t)(c.off + k)];
    }
}

void plan_or_fail(ace_ctx *ctx, int64_t n, int64_t nf, const int64_t *off, const int64_t *idx,
                  const int64_t *perm, CvPlan &pl) {
  const std::string why = cv_plan(n, nf, off, idx, perm, cv_wg_max(), &pl);
  if (why.empty()) return;
  ctx->err = why;
  throw Fail{ACE_ERR_ARG};
}

}  // namespace

extern "C" {

int ace_model_cv(ace_model *m, const double *theta, int64_t nf, const int64_t *off,
                 const int64_t *idx, double mean_y, double std_y, double *map, double *var,
                 double *resid, double *lpd, double *mahal, int *status) {
  if (!m) return ACE_ERR_ARG;
  ace_ctx *ctx = m->ctx;
  ACE_TRY
  ck(ctx, hipSetDevice(ctx->device), "hipSetDevice");
  arg(ctx, theta && nf >= 1 && off && idx, "bad shape / null argument");
  refuse(ctx, !m->shard, "cv: sharded models are not supported (single GPU only)");
  arg(ctx, m->has_data, "ace_model_set_data() not called");
  refuse(ctx, m->has_inverse,
         "cv: the model holds no resident inverse (call ace_model_para_update() first)");
  const int64_t n = m->n;
  CvPlan pl;
  plan_or_fail(ctx, n, nf, off, idx, m->perm.empty() ? nullptr : m->perm.data(), pl);
  hipStream_t st = ctx->stream;
  // alpha = A^-1 y - mu A^-1 1 from the swept AUG rows, mu the caller's
  DBuf dalpha, dscal;
  alloc(ctx, dalpha, (size_t)n * sizeof(double), "alloc alpha");
  alloc(ctx, dscal, 8 * sizeof(double), "alloc scalars");
  ck(ctx, launch_alpha_from_aug(m->sw.A.d(), m->naug, m->npad, n, theta[1], 0, dalpha.d(),
                                dscal.d(), st),
     "alpha");
  CvHost h;
  cv_core(ctx, m->sw.A.d(), m->naug, -1.0, dalpha.d(), pl, h);  // -A^-1 is stored
  std::vector<double> hy;
  if (map) {  // y in the device's order
    hy.resize((size_t)n);
    download(ctx, hy.data(), m->y.d(), (size_t)n, "download y");
    sync(ctx);
  }
  const double log2pi = std::log(2.0 * M_PI);
  for (int64_t f = 0; f < nf; ++f) {
    const CvFold &c = pl.folds[(size_t)f];
    for (int64_t k = 0; k < c.m; ++k) {
      const size_t to = (size_t)(c.off + pl.scatter[(size_t)(c.off + k)]);
      if (map) map[to] = mean_y + std_y * (hy[(size_t)pl.rows[(size_t)(c.off + k)]] - h.r[to]);
      if (var) var[to] = std_y * std_y * h.v[to];
      if (resid) resid[to] = std_y * h.r[to];
    }
    const double mm = (double)c.m;
    if (lpd)
      lpd[f] = -0.5 * h.mahal[(size_t)f] + 0.5 * h.logdet[(size_t)f] - 0.5 * mm * log2pi -
               mm * std::log(std_y);
    if (mahal) mahal[f] = h.mahal[(size_t)f];
    if (status) status[f] = h.status[(size_t)f];
  }
  return ACE_OK;
  ACE_CATCH
}

int ace_cv_from_inverse(ace_ctx *ctx, int64_t n, const double *P, int64_t ldp,
                        const double *alpha, int64_t nf, const int64_t *off, const int64_t *idx,
                        double *resid, double *var, double *logdet, double *mahal, int *status) {
  if (!ctx) return ACE_ERR_ARG;
  ACE_TRY
  ck(ctx, hipSetDevice(ctx->device), "hipSetDevice");
  arg(ctx, n >= 1 && P && alpha && ldp >= n && nf >= 1 && off && idx, "bad shape / null argument");
  CvPlan pl;
  plan_or_fail(ctx, n, nf, off, idx, nullptr, pl);
  std::vector<double> hp((size_t)(n * n));
  for (int64_t c = 0; c < n; ++c) std::copy(P + c * ldp, P + c * ldp + n, hp.begin() + c * n);
  DBuf dP, dalpha;
  upload(ctx, dP, hp.data(), hp.size(), "upload P");
  upload(ctx, dalpha, alpha, (size_t)n, "upload alpha");
  CvHost h;
  cv_core(ctx, dP.d(), n, 1.0, dalpha.d(), pl, h);
  if (resid) std::copy(h.r.begin(), h.r.end(), resid);
  if (var) std::copy(h.v.begin(), h.v.end(), var);
  if (logdet) std::copy(h.logdet.begin(), h.logdet.end(), logdet);
  if (mahal) std::copy(h.mahal.begin(), h.mahal.end(), mahal);
  if (status) std::copy(h.status.begin(), h.status.end(), status);
  return ACE_OK;
  ACE_CATCH
}

}  // extern "C"
