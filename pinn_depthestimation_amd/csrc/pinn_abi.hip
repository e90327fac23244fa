// pinn_abi.hip — extern "C" entry points of libpinn_hip.so (see include/pinn_hip.h)
// and the engine dispatch.  No torch types, no exceptions, no allocation.
#include <string.h>
#include <mutex>
#include <utility>
#include <vector>
#include "common.h"
#include "reduce_adam.h"
#include "adam_ext.h"
#include "balance.h"
#include "residuals.h"
#include "lbfgs_loop.h"
#include "lbfgs_line_search.h"

namespace pinn {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// The only process-wide state of the library: immutable facts about devices / kernels, filled on first use.
namespace {
std::mutex g_cache_mu;
constexpr int MAX_DEVICES = 64;
int g_cus[MAX_DEVICES];                                              // 0 = not yet asked
struct LdsKey { const void* fn; int dev; size_t bytes; };
std::vector<LdsKey> g_lds_set;
}  // namespace

int device_cu_count() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) return 256;
  std::lock_guard<std::mutex> lk(g_cache_mu);
  if (g_cus[dev] == 0) {
    int v = 0;
    g_cus[dev] = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256;
  }
  return g_cus[dev];
}

int ensure_dynamic_lds(const void* kernel, size_t lds_bytes) {
  if (lds_bytes <= 64 * 1024) return PINN_OK;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { set_error("hipGetDevice failed"); return PINN_ERR_LAUNCH; }
  std::lock_guard<std::mutex> lk(g_cache_mu);
  for (LdsKey& k : g_lds_set)
    if (k.fn == kernel && k.dev == dev) {
      if (k.bytes >= lds_bytes) return PINN_OK;
      hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
      if (e != hipSuccess) { set_error("hipFuncSetAttribute(%zu B LDS): %s", lds_bytes, hipGetErrorString(e)); return PINN_ERR_LAUNCH; }
      k.bytes = lds_bytes;
      return PINN_OK;
    }
  hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  if (e != hipSuccess) { set_error("hipFuncSetAttribute(%zu B LDS): %s", lds_bytes, hipGetErrorString(e)); return PINN_ERR_LAUNCH; }
  g_lds_set.push_back(LdsKey{kernel, dev, lds_bytes});
  return PINN_OK;
}

int make_net(const pinn_desc* d, Net* n) {
  if (!d) { set_error("desc is NULL"); return PINN_ERR_INVALID; }
  if (d->d_in < 1 || d->d_out < 1 || d->n_hidden < 1 || d->width < 1) {
    set_error("bad network shape d_in=%d d_out=%d hidden=%d width=%d", d->d_in, d->d_out, d->n_hidden, d->width);
    return PINN_ERR_INVALID;
  }
  if (d->k < 0 || d->k > PINN_MAX_DIRS) { set_error("k=%d outside 0..%d", d->k, PINN_MAX_DIRS); return PINN_ERR_INVALID; }
  if (d->activation != PINN_ACT_TANH && d->activation != PINN_ACT_LEAKY_RELU && d->activation != PINN_ACT_SIN_TANH) {
    // mirrors the ValueError of dnn.py:23 for an unknown init_type
    set_error("invalid activation %d (0 = tanh/'xavier', 1 = leaky_relu/'kaiming', 2 = sine first layer then tanh)", d->activation);
    return PINN_ERR_INVALID;
  }
  n->d_in = d->d_in; n->d_out = d->d_out; n->L = d->n_hidden; n->W = d->width;
  n->k = d->k; n->K1 = 1 + d->k; n->act = d->activation; n->n_lin = d->n_hidden + 1;
  if (d->precision != PINN_PREC_F32 && d->precision != PINN_PREC_BF16) {
    set_error("invalid precision %d", d->precision); return PINN_ERR_INVALID;
  }
  n->prec = d->precision;
  if (d->engine < PINN_ENGINE_AUTO || d->engine > PINN_ENGINE_FUSED_BATCH) { set_error("invalid engine %d", d->engine); return PINN_ERR_INVALID; }
  n->fused_kernel = d->engine == PINN_ENGINE_FUSED_TILE ? FUSED_KERNEL_TILE
                  : d->engine == PINN_ENGINE_FUSED_COOP ? FUSED_KERNEL_COOP
                  : d->engine == PINN_ENGINE_FUSED_BATCH ? FUSED_KERNEL_BATCH : FUSED_KERNEL_AUTO;
  if (!(d->dropout_p >= 0.f && d->dropout_p < 1.f)) { set_error("dropout_p=%g outside [0, 1)", (double)d->dropout_p); return PINN_ERR_INVALID; }
  n->drop_p = d->dropout_p; n->drop_seed = d->dropout_seed; n->drop_thresh = dropout_threshold(d->dropout_p);
  if (n->drop_p > 0.f && n->drop_thresh == 0) n->drop_thresh = 1;   // (0 means "off" in the kernels)
  for (int j = 0; j < PINN_MAX_DIRS; ++j) {
    n->dir_col[j] = j < d->k ? d->dir_col[j] : -1;
    if (j < d->k && (d->dir_col[j] < 0 || d->dir_col[j] >= d->d_in)) {
      set_error("dir_col[%d]=%d outside the %d input columns", j, d->dir_col[j], d->d_in);
      return PINN_ERR_INVALID;
    }
  }
  return PINN_OK;
}

// the engine desc asks for, with the fused engine's kernel choices (FUSED_TILE / _COOP / _BATCH) folded into FUSED
static int asked_engine(const pinn_desc* d) {
  return (d->engine == PINN_ENGINE_FUSED_TILE || d->engine == PINN_ENGINE_FUSED_COOP || d->engine == PINN_ENGINE_FUSED_BATCH)
             ? PINN_ENGINE_FUSED : d->engine;
}

// 1 = generic, 2 = fused, 3 = wide
static int pick_engine(const pinn_desc* d, const Net& n, bool want_grad, int* rc) {
  *rc = PINN_OK;
  const int asked = asked_engine(d);
  if (n.drop_p > 0.f) {     // training-mode dropout: the fused tile kernel for gradient passes at padded width 64
                            // (pinn_fused_tile.hip, TF_DROP), the generic engine's kernels for everything else
    if (n.prec != PINN_PREC_F32) { set_error("dropout_p > 0 is implemented in fp32 only"); *rc = PINN_ERR_UNSUPPORTED; return PINN_ENGINE_GENERIC; }
    const bool fused_ok = fused_supports(n, want_grad);
    if (asked == PINN_ENGINE_FUSED && !fused_ok) {
      set_error("dropout_p > 0 on the fused engine: gradient passes of tanh networks of hidden width 33..64 only; this request "
                "runs on the generic engine (engine AUTO or GENERIC)");
      *rc = PINN_ERR_UNSUPPORTED;
    } else if (asked == PINN_ENGINE_WIDE) {
      set_error("dropout_p > 0 runs on the generic engine (engine AUTO or GENERIC), not on engine %d", d->engine);
      *rc = PINN_ERR_UNSUPPORTED;
    }
    return (asked == PINN_ENGINE_AUTO || asked == PINN_ENGINE_FUSED) && fused_ok ? PINN_ENGINE_FUSED : PINN_ENGINE_GENERIC;
  }
  if (n.prec == PINN_PREC_BF16) {   // bf16 operands exist on the wide engine only
    if (n.act == PINN_ACT_SIN_TANH) {
      set_error("precision bf16 is implemented on the wide engine only, which has no kernel for the sine first layer "
                "(activation 2): use precision fp32");
      *rc = PINN_ERR_UNSUPPORTED;
      return PINN_ENGINE_WIDE;
    }
    if ((asked != PINN_ENGINE_AUTO && asked != PINN_ENGINE_WIDE) || !wide_supports(n)) {
      set_error("precision bf16 is implemented on the wide engine (64 < width <= 256, tanh, k in {0,2,3}) only");
      *rc = PINN_ERR_UNSUPPORTED;
    }
    return PINN_ENGINE_WIDE;
  }
  if (asked == PINN_ENGINE_GENERIC) return PINN_ENGINE_GENERIC;
  if (asked == PINN_ENGINE_FUSED || asked == PINN_ENGINE_WIDE) {
    const bool ok = asked == PINN_ENGINE_FUSED ? fused_supports(n, want_grad) : wide_supports(n);
    if (!ok && n.act == PINN_ACT_SIN_TANH) {
      // the sine first layer: the tile kernel's own instances only (pinn_fused_tile.hip, TF_SIN)
      const char* why = asked == PINN_ENGINE_WIDE ? "the wide engine has no kernel for it"
                      : n.fused_kernel == FUSED_KERNEL_COOP ? "engine FUSED_COOP: the cooperative kernel has no instance for it (use AUTO, FUSED or FUSED_TILE)"
                      : n.fused_kernel == FUSED_KERNEL_BATCH ? "engine FUSED_BATCH: the batch kernel has no instance for it (use AUTO, FUSED or FUSED_TILE)"
                      : "the tile kernel's sine instances serve width <= 64, d_in and d_out <= 16, k in {0, 2, 3}, no dropout";
      set_error("the sine first layer (activation 2): %s (width %d, d_in %d, d_out %d, k %d, gradient %d); engine AUTO or GENERIC "
                "runs this request on the generic engine", why, n.W, n.d_in, n.d_out, n.k, (int)want_grad);
      *rc = PINN_ERR_UNSUPPORTED;
    } else if (!ok) {
      set_error("%s engine does not support this request (width %d, d_in %d, d_out %d, k %d, act %d, gradient %d)",
                asked == PINN_ENGINE_FUSED ? "fused" : "wide", n.W, n.d_in, n.d_out, n.k, n.act, (int)want_grad);
      *rc = PINN_ERR_UNSUPPORTED;
    }
    return asked;
  }
  if (fused_supports(n, want_grad)) return PINN_ENGINE_FUSED;
  if (wide_supports(n)) return PINN_ENGINE_WIDE;
  return PINN_ENGINE_GENERIC;
}

// pinn_jet_backward: GENERIC or FUSED (the external-adjoint instances of the tile or the batch kernel: which of the two,
// fused_jet_backward_kernel says; whether the call is served does not depend on the fused kernel desc.engine names).  AUTO takes the MFMA path where it exists and the generic engine for everything else (k = 1 with gdY, dropout,
// width > 64, d_in / d_out > 16, bf16); an explicit FUSED request the path does not serve is refused, WIDE always.
static int pick_jet_backward_engine(const pinn_desc* d, const Net& n, int* rc) {
  *rc = PINN_OK;
  const int asked = asked_engine(d);
  if (asked == PINN_ENGINE_GENERIC) return PINN_ENGINE_GENERIC;
  if (asked == PINN_ENGINE_WIDE) {
    set_error("pinn_jet_backward is not implemented on the wide engine: use engine AUTO, GENERIC or FUSED");
    *rc = PINN_ERR_UNSUPPORTED;
    return PINN_ENGINE_GENERIC;
  }
  const char* why = fused_tile_refusal(TILE_ADJ, n);
  if (asked == PINN_ENGINE_FUSED && why) {
    set_error("pinn_jet_backward on the fused engine: %s (width %d, d_in %d, d_out %d, k %d, hidden layers %d); "
              "engine AUTO or GENERIC runs this request on the generic engine", why, n.W, n.d_in, n.d_out, n.k, n.L);
    *rc = PINN_ERR_UNSUPPORTED;
  }
  return why ? PINN_ENGINE_GENERIC : PINN_ENGINE_FUSED;
}

// engine e's member of a trio of functions with one signature (fused_X, wide_X, generic_X of common.h)
template <class F>
static F* on_engine(int e, F* fused, F* wide, F* generic) {
  return e == PINN_ENGINE_FUSED ? fused : e == PINN_ENGINE_WIDE ? wide : generic;
}

static int64_t engine_workspace_bytes(int engine, const Net& n, int64_t N) {
  return on_engine(engine, fused_workspace_bytes, wide_workspace_bytes, generic_workspace_bytes)(n, N);
}

// A request with the corrected radiation stress (spec.flags bit 0 -> RES_PE_CORRECTED, check_spec) is served on the engine
// pick_engine chose for the descriptor (*e) or refused with the reason — never moved to another engine, whose workspace
// pinn_query_workspace (which does not see the spec) may not have covered.  The one exception: with dropout_p > 0 the fused
// dropout instances count as absent and AUTO runs the generic engine, which the query of a dropout descriptor covers
// already (its forward calls run there).  Pure host logic: nothing touches a device before a refusal.
// The wave closure (bits 0 and 1 -> RES_PE_WAVE) follows the same rule with its own instances of the tile kernel only: the
// batch and the cooperative kernel, when the descriptor forces them, are refused, and so is an eighth fidelity column on the
// fused engine (the fifth term's partial sum takes that column's slot: fused_kernel.h, term_slot).
// rc_pick: pick_engine's own verdict on the descriptor (its reason is in the error buffer); where the closure's rule has
// nothing to add, a wave request's refusal repeats that reason under the closure's name (name_refusal).
static int name_refusal(const char* name, int rc) {
  char picked[sizeof(g_err)];
  snprintf(picked, sizeof(picked), "%s", g_err);
  set_error("%s: %.300s; use engine GENERIC", name, picked);
  return rc;
}
static int corrected_engine(const pinn_desc* desc, const Net& n, const LossReq& rq, int* e, int rc_pick) {
  if (rq.kind == 1 || !is_pe_closure(rq.spec.residual_id)) return PINN_OK;
  const bool wave = rq.spec.residual_id == RES_PE_WAVE;
  const char* name = pe_closure_name(wave);
  if (*e == PINN_ENGINE_WIDE) {
    set_error("%s is not implemented on the wide engine (width 65..256, "
              "bf16 operands): width %d, precision %d; use engine GENERIC in fp32", name, n.W, n.prec);
    return PINN_ERR_UNSUPPORTED;
  }
  if (wave && *e == PINN_ENGINE_FUSED && (n.fused_kernel == FUSED_KERNEL_BATCH || n.fused_kernel == FUSED_KERNEL_COOP)) {
    set_error("%s has instances of the tile kernel only: engine %s has none; use engine AUTO, FUSED, FUSED_TILE or GENERIC",
              name, n.fused_kernel == FUSED_KERNEL_BATCH ? "FUSED_BATCH" : "FUSED_COOP");
    return PINN_ERR_UNSUPPORTED;
  }
  if (*e == PINN_ENGINE_FUSED && n.drop_p > 0.f && asked_engine(desc) == PINN_ENGINE_AUTO) *e = PINN_ENGINE_GENERIC;
  // ... and with the sine first layer: the fused engine has no EPI_PEC sine instance, AUTO runs the generic engine, which the
  // query of a sine descriptor under AUTO covers (pinn_query_workspace)
  if (*e == PINN_ENGINE_FUSED && n.act == PINN_ACT_SIN_TANH && asked_engine(desc) == PINN_ENGINE_AUTO) *e = PINN_ENGINE_GENERIC;
  if (*e == PINN_ENGINE_FUSED) {
    if (const char* why = fused_corrected_refusal(n)) {
      set_error("%s %s (activation %d, k %d, dropout_p %g)", name, why, n.act, n.k, (double)n.drop_p);
      return PINN_ERR_UNSUPPORTED;
    }
    if (wave && rc_pick) return name_refusal(name, rc_pick);
    if (wave && !rc_pick && rq.kind == 2 && rq.n_cols > WAVE_MAX_COLS) {
      set_error("%s with %d fidelity columns on the fused engine: the fifth term's partial sum takes the last column's slot, "
                "at most %d columns are served; use engine GENERIC", name, rq.n_cols, WAVE_MAX_COLS);
      return PINN_ERR_UNSUPPORTED;
    }
  }
  if (wave && rc_pick) return name_refusal(name, rc_pick);
  return PINN_OK;
}

// runs rq on the engine pick_engine() chooses for it
static int run_loss(const pinn_desc* desc, const Net& n, bool want_grad, const LossReq& rq, const float* params,
                    const float* X, int64_t N, void* ws, int64_t ws_bytes, void* stream) {
  int rc; int e = pick_engine(desc, n, want_grad, &rc);
  if (int rcc = corrected_engine(desc, n, rq, &e, rc)) return rcc;
  if (rc) return rc;
  return on_engine(e, fused_loss, wide_loss, generic_loss)(n, rq, params, X, N, ws, ws_bytes, (hipStream_t)stream);
}

// the fidelity columns: each must name an output of the network; copied into rq->out_col
static int set_out_cols(const Net& n, int n_cols, const int32_t* out_col, LossReq* rq) {
  for (int j = 0; j < n_cols; ++j) {
    if (out_col[j] < 0 || out_col[j] >= n.d_out) { set_error("out_col[%d]=%d out of range", j, out_col[j]); return PINN_ERR_INVALID; }
    rq->out_col[j] = out_col[j];
  }
  return PINN_OK;
}

// What each residual uses: its first `roles` output roles and `dirs` direction roles; how many loss terms and per-point
// fields it has (pinn_hip.h's numbers: ResContinuity::NT is the kernels' 3 for both continuity residuals).  Null for an
// id that names no residual.
struct ResidualInfo { int id, roles, dirs, terms, fields; };
static const ResidualInfo* residual_info(int id) {
  static const ResidualInfo table[] = {{PINN_RES_NAVIER_STOKES, 4, 3, PINN_NS_TERMS, PINN_NS_FIELDS},
                                       {PINN_RES_PHYSICS_EQUATION, 6, 2, PINN_PE_TERMS, PINN_PE_FIELDS},
                                       {PINN_RES_CONTINUITY_FTEMP, 3, 2, PINN_CF_TERMS, PINN_CF_FIELDS},
                                       {PINN_RES_CONTINUITY_ONLY, 3, 2, PINN_CO_TERMS, PINN_CO_FIELDS}};
  for (const ResidualInfo& r : table) if (r.id == id) return &r;
  return nullptr;
}
// (-1 for an id that names no residual)
static int residual_terms(int id) { const ResidualInfo* r = residual_info(id); return r ? r->terms : -1; }
// the caller's spec asks for the wave closure (flags bits 0 and 1 on physics_equation; check_spec refuses bit 1 alone)
static bool is_wave_spec(const pinn_residual_spec* sp) { return sp->residual_id == PINN_RES_PHYSICS_EQUATION && (sp->flags & 2); }
// ... the terms (and fields) of the caller's spec: the wave closure adds two to physics_equation's
static int spec_terms(const pinn_residual_spec* sp) { return is_wave_spec(sp) ? PINN_PEW_TERMS : residual_terms(sp->residual_id); }
static int residual_dirs(int id) { const ResidualInfo* r = residual_info(id); return r ? r->dirs : -1; }
// (the terms a point weight applies to: the residual's terms that are sums of a squared field, pinn_hip.h's n_w)
static int residual_n_weighted(int id) { const ResidualInfo* r = residual_info(id); return !r ? -1 : r->terms < r->fields ? r->terms : r->fields; }

// the entries that evaluate the residual on the network's own jet: k must be its number of directions (note: "" or what
// the message adds after the residual's id)
static int check_k(const char* who, const Net& n, const pinn_residual_spec* spec, const char* note) {
  const int dirs = residual_dirs(spec->residual_id);
  if (n.k == dirs) return PINN_OK;
  set_error("%s: the network carries k = %d tangent directions, residual %d%s has %d (k must equal the residual's number of "
            "directions)", who, n.k, spec->residual_id, note, dirs);
  return PINN_ERR_UNSUPPORTED;
}

// Checks the roles the residual USES (its first nr output roles, nd direction roles) and returns in *norm a copy whose
// unused entries are inert: out_col = -1 (matches no output column), dir_of = -1 (quantity 0 is never a direction).
// The engines' per-lane scatter tables are built by searching ALL PINN_MAX_ROLES entries for "which role lives in
// this column"; an unused entry left at 0 (zero-initialised structs: every caller) claimed output column 0 whenever no
// real role sat there, and the output adjoint of that column was read from beyond the roles' rows.
static int check_spec(const Net& n, const pinn_residual_spec* sp, pinn_residual_spec* norm) {
  if (!sp) { set_error("spec is NULL"); return PINN_ERR_INVALID; }
  // (RES_PE_CORRECTED, the library's own id of the corrected physics_equation, is no id a caller may pass: the table
  // holds the four public ones)
  const ResidualInfo* ri = residual_info(sp->residual_id);
  if (!ri) { set_error("unknown residual_id %d", sp->residual_id); return PINN_ERR_INVALID; }
  if (is_wave_spec(sp)) {   // flags bit 1: the wave closure needs the corrected stress and its two parameters
    if (!(sp->flags & 1)) {
      set_error("spec.flags bit 1 (the wave closure) without bit 0: the dispersion and wave-energy terms close the corrected "
                "radiation stress (flags = 3)");
      return PINN_ERR_INVALID;
    }
    if (!(sp->param[0] > 0.f) || !(sp->param[1] > 0.f)) {
      set_error("the wave closure (spec.flags bit 1) needs param[0] = omega > 0 and param[1] = gamma > 0 (got %g, %g)",
                (double)sp->param[0], (double)sp->param[1]);
      return PINN_ERR_INVALID;
    }
  }
  const int nr = ri->roles, nd = ri->dirs;
  for (int r = 0; r < nr; ++r)
    if (sp->out_col[r] < 0 || sp->out_col[r] >= n.d_out) {
      set_error("out_col[%d]=%d outside the %d output columns", r, sp->out_col[r], n.d_out);
      return PINN_ERR_INVALID;
    }
  for (int d = 0; d < nd; ++d)
    if (sp->dir_of[d] < 0 || sp->dir_of[d] >= n.k) {
      set_error("dir_of[%d]=%d but the network carries %d tangent directions", d, sp->dir_of[d], n.k);
      return PINN_ERR_INVALID;
    }
  *norm = *sp;
  for (int r = nr; r < PINN_MAX_ROLES; ++r) norm->out_col[r] = -1;
  for (int d = nd; d < PINN_MAX_DIRS; ++d) norm->dir_of[d] = -1;
  // flags bit 0 on physics_equation: the corrected radiation stress, carried as an id of its own from here on
  if (sp->residual_id == PINN_RES_PHYSICS_EQUATION && (sp->flags & 1)) norm->residual_id = RES_PE_CORRECTED;
  // ... and bits 0 and 1: the wave closure
  if (is_wave_spec(sp)) norm->residual_id = RES_PE_WAVE;
  return PINN_OK;
}

// The part of a loss request that every entry with a residual builds alike, into a zeroed *rq: the normalised spec and its
// number of terms; the residual on points [0, n_res) and the n_cols fidelity columns on the rest (n_res < 0: both on every
// point), with the range rules of n_res and n_cols (min_cols: 1 where the entry has no meaning for none); the columns
// (out_col == NULL is left to the entry's own NULL checks, which follow); kind and n_split.  A residual-only entry
// passes n_res = N and no columns.  The entry adds its pointers.
static int build_request(const Net& n, const pinn_residual_spec* spec, int64_t N, int64_t n_res, int min_cols, int32_t n_cols,
                         const int32_t* out_col, LossReq* rq) {
  memset(rq, 0, sizeof(*rq));
  if (int rc = check_spec(n, spec, &rq->spec)) return rc;
  rq->n_terms = spec_terms(spec);
  if (n_res > N) { set_error("n_res=%lld exceeds N=%lld", (long long)n_res, (long long)N); return PINN_ERR_INVALID; }
  if (n_cols < min_cols || n_cols > PINN_MAX_ROLES) {
    set_error("n_cols=%d outside %d..%d", n_cols, min_cols, PINN_MAX_ROLES); return PINN_ERR_INVALID;
  }
  if (n_cols == 0 && n_res != N) { set_error("no fidelity columns: n_res must equal N"); return PINN_ERR_INVALID; }
  rq->n_cols = n_cols;
  if (out_col) { if (int rc = set_out_cols(n, n_cols, out_col, rq)) return rc; }
  if (n_res == N) { rq->kind = 0; rq->n_split = -1; }      // residual term only
  else { rq->kind = 2; rq->n_split = n_res < 0 ? -1 : n_res; }
  return PINN_OK;
}

// the folded update of a loss + gradient pass from the caller's state (its moments and step were checked by the entry)
static int adam_req(const pinn_adam_state* adam, float* params, AdamReq* a) {
  if (adam->n_loss_rows < 0 || adam->n_loss_rows > 8 || (adam->n_loss_rows > 0 && (!adam->loss_rows || !adam->losses))) {
    set_error("bad loss_rows arguments"); return PINN_ERR_INVALID;
  }
  a->params = params; a->m = adam->m; a->v = adam->v;
  a->c = adam_scalars(adam->lr, adam->beta1, adam->beta2, adam->eps, adam->step);
  a->packed_valid = adam->packed_valid != 0;
  a->n_loss_rows = adam->n_loss_rows; a->loss_rows = adam->loss_rows; a->losses = adam->losses;
  return PINN_OK;
}

// the state of iteration i of a host-side loop over the folded update: its step and learning rate, the packed weights left
// by the iteration before, and its `stride` floats of the losses array
static pinn_adam_state adam_state_at(const pinn_adam_state* adam, int32_t i, const double* lr, int64_t stride) {
  pinn_adam_state st = *adam;
  st.step = adam->step + i; st.lr = lr[i];
  st.packed_valid = (i > 0 || adam->packed_valid) ? 1 : 0;
  if (adam->n_loss_rows > 0 && adam->losses) st.losses = adam->losses + (int64_t)i * stride;
  return st;
}

// The one column-sum kernel of the library: the fused, wide and generic hosts launch it through reduce_sums (reduce_adam.h).
__global__ void k_reduce_sums(const float* __restrict__ rows, int64_t n_rows, int stride, int col0, float* __restrict__ out) {
  const double v = column_sum(rows, n_rows, stride, col0 + blockIdx.x);
  if (threadIdx.x == 0) out[blockIdx.x] = (float)v;
}
void reduce_sums(const float* rows, int64_t n_rows, int stride, int col0, int n, float* out, hipStream_t s) {
  hipLaunchKernelGGL(k_reduce_sums, dim3(n), dim3(256), 0, s, rows, n_rows, stride, col0, out);
}

__global__ void k_reduce_sums_add(const float* __restrict__ rows, int64_t n_rows, int stride, int col0, float* __restrict__ out) {
  const double v = column_sum(rows, n_rows, stride, col0 + blockIdx.x);
  if (threadIdx.x == 0) out[blockIdx.x] += (float)v;
}
void reduce_sums_add(const float* rows, int64_t n_rows, int stride, int col0, int n, float* out, hipStream_t s) {
  hipLaunchKernelGGL(k_reduce_sums_add, dim3(n), dim3(256), 0, s, rows, n_rows, stride, col0, out);
}

__global__ void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                       float* __restrict__ v, int64_t P, AdamScalars c) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < P) p[i] = adam_update(p[i], g[i], m[i], v[i], c);
}

// The *_point entries' copy-in / copy-out (the residuals of residuals.h at ONE point, on the host): the flat jet v ->
// jet[1 + ND][NR], body(jet, gj), and, where body says it formed the adjoint, gj -> the flat g.
template <class R, class F>
static void point_jet(const float* v, float* g, F body) {
  float jet[1 + R::ND][R::NR], gj[1 + R::ND][R::NR];
  for (int c = 0; c <= R::ND; ++c)
    for (int r = 0; r < R::NR; ++r) jet[c][r] = v[c * R::NR + r];
  if (!body(jet, gj)) return;
  for (int c = 0; c <= R::ND; ++c)
    for (int r = 0; r < R::NR; ++r) g[c * R::NR + r] = gj[c][r];
}

}  // namespace pinn

using namespace pinn;

extern "C" {

int32_t pinn_version(void) { return PINN_ABI_VERSION; }
int32_t pinn_dropout_keep(uint32_t seed, int32_t layer, int32_t feature, int64_t point, float p) {
  return dropout_bits(seed, (uint32_t)layer, (uint32_t)feature, (uint64_t)point) >= dropout_threshold(p) ? 1 : 0;
}
const char* pinn_last_error(void) { return g_err; }

int32_t pinn_pe_corrected_point(const float v[18], const float scale[3], float fields[3], float g[18]) {
  typedef ResPhysicsEquationCorrected R;
  if (!v || !fields) { set_error("NULL pointer argument"); return PINN_ERR_INVALID; }
  point_jet<R>(v, g, [&](const float (&jet)[1 + R::ND][R::NR], float (&gj)[1 + R::ND][R::NR]) {
    float sq[R::NT];
    R::fields(jet, R::Closure(), *reinterpret_cast<float (*)[R::NF]>(fields));
    if (!scale || !g) return false;
    R::eval<true>(jet, R::Closure(), scale, gj, sq);
    return true;
  });
  return PINN_OK;
}

int32_t pinn_pe_wave_point(const float v[18], float omega, float gamma, const float scale[5], float fields[5], float g[18]) {
  typedef ResPhysicsEquationWave R;
  if (!v || !fields) { set_error("NULL pointer argument"); return PINN_ERR_INVALID; }
  if (!(omega > 0.f) || !(gamma > 0.f)) {
    set_error("pinn_pe_wave_point: the wave closure needs omega > 0 and gamma > 0 (got %g, %g)", (double)omega, (double)gamma);
    return PINN_ERR_INVALID;
  }
  const R::Closure cl = {omega, gamma};
  point_jet<R>(v, g, [&](const float (&jet)[1 + R::ND][R::NR], float (&gj)[1 + R::ND][R::NR]) {
    float sq[R::NT];
    R::fields(jet, cl, *reinterpret_cast<float (*)[R::NF]>(fields));
    if (!scale || !g) return false;
    R::eval<true>(jet, cl, scale, gj, sq);
    return true;
  });
  return PINN_OK;
}

int32_t pinn_param_count(const pinn_desc* desc, int64_t* count) {
  Net n; int rc = make_net(desc, &n); if (rc) return rc;
  if (!count) { set_error("count is NULL"); return PINN_ERR_INVALID; }
  *count = n.n_params();
  return PINN_OK;
}

int32_t pinn_query_workspace(const pinn_desc* desc, int64_t N, int64_t* bytes) {
  Net n; int rc = make_net(desc, &n); if (rc) return rc;
  if (!bytes || N < 0) { set_error("bad arguments"); return PINN_ERR_INVALID; }
  // one workspace must serve every call on this network: gradient calls that AUTO routes to another engine than the
  // forward (k = 1 networks: fused forward, generic gradient), and the calls that run the network WITHOUT its tangents
  // (pinn_forward, pinn_mse_loss_grad, pinn_jet_backward without gdY: k = 0), which may land on yet another engine
  // (k = 1 at width 65..256: jets on the generic kernels, plain forwards on the wide engine)
  auto need = [&](const Net& nn, int* err) -> int64_t {
    auto ws_of = [&](int e) { return engine_workspace_bytes(e, nn, N); };
    int rc1 = PINN_OK, rc2 = PINN_OK;
    const int e = pick_engine(desc, nn, false, &rc1);
    const int eg = pick_engine(desc, nn, true, &rc2);
    if (rc1 && rc2) { *err = rc1; return -1; }      // neither kind of call is served on the engine asked for
    int64_t b = rc1 ? -1 : ws_of(e);
    if (rc2 == PINN_OK && (rc1 || eg != e)) { const int64_t bg = ws_of(eg); if (bg > b) b = bg; }
    if (b >= 0 && nn.act == PINN_ACT_SIN_TANH && asked_engine(desc) == PINN_ENGINE_AUTO) {
      // the sine first layer under AUTO: a corrected-radiation-stress loss request runs on the generic engine (corrected_engine)
      const int64_t bg = generic_workspace_bytes(nn, N);
      if (bg > b) b = bg;
    }
    if (b >= 0) {   // pinn_jet_backward picks its engine by its own rule (a request refused there fails by itself)
      int rcj = PINN_OK;
      const int ej = pick_jet_backward_engine(desc, nn, &rcj);
      if (rcj == PINN_OK) {
        Net t = nn; t.fused_kernel = FUSED_KERNEL_TILE;
        const int64_t bj = ej == PINN_ENGINE_FUSED ? fused_workspace_bytes(t, N) : generic_workspace_bytes(nn, N);
        if (bj > b) b = bj;
      }
    }
    return b;
  };
  int64_t b = need(n, &rc);
  if (b < 0 && rc) return rc;
  if (n.k > 0) {
    Net n0 = n; n0.k = 0; n0.K1 = 1;
    int rc0 = PINN_OK;
    const int64_t b0 = need(n0, &rc0);               // (refused on the engine asked for: those calls fail by themselves)
    if (b0 > b) b = b0;
  }
  if (b < 0) { set_error("network not supported"); return PINN_ERR_UNSUPPORTED; }
  *bytes = b;
  return PINN_OK;
}

static int32_t forward_impl(const pinn_desc* desc, const float* params, const float* X, int64_t N, float* Y,
                            float* dY, void* ws, int64_t ws_bytes, void* stream, bool jet) {
  Net n; int rc = make_net(desc, &n); if (rc) return rc;
  if (!params || (!X && N > 0) || N < 0 || (!Y && N > 0) || (jet && !dY && N > 0)) { set_error("NULL pointer argument"); return PINN_ERR_INVALID; }
  if (N == 0) return PINN_OK;
  if (!jet) { n.k = 0; n.K1 = 1; dY = nullptr; }
  if (jet && n.k == 0) { set_error("forward_jet needs k >= 1"); return PINN_ERR_INVALID; }
  const int e = pick_engine(desc, n, false, &rc); if (rc) return rc;
  return on_engine(e, fused_forward, wide_forward, generic_forward)(n, params, X, N, Y, dY, ws, ws_bytes, (hipStream_t)stream);
}

int32_t pinn_forward(const pinn_desc* desc, const float* params, const float* X, int64_t N, float* Y, void* ws,
                     int64_t ws_bytes, void* stream) {
  return forward_impl(desc, params, X, N, Y, nullptr, ws, ws_bytes, stream, false);
}

int32_t pinn_forward_jet(const pinn_desc* desc, const float* params, const float* X, int64_t N, float* Y,
                         float* dY, void* ws, int64_t ws_bytes, void* stream) {
  return forward_impl(desc, params, X, N, Y, dY, ws, ws_bytes, stream, true);
}

int32_t pinn_jet_backward(const pinn_desc* desc, const float* params, const float* X, int64_t N, const float* gY,
                          const float* gdY, float* grad_flat, void* ws, int64_t ws_bytes, void* stream) {
  Net n; int rc = make_net(desc, &n); if (rc) return rc;
  if (!params || (!X && N > 0) || N < 0 || !grad_flat || (!gY && !gdY && N > 0)) { set_error("NULL pointer argument"); return PINN_ERR_INVALID; }
  if (N == 0) return PINN_OK;
  if (!gdY) { n.k = 0; n.K1 = 1; }
  const int e = pick_jet_backward_engine(desc, n, &rc); if (rc) return rc;
  return e == PINN_ENGINE_FUSED ? fused_jet_backward(n, params, X, N, gY, gdY, grad_flat, ws, ws_bytes, (hipStream_t)stream)
                                : generic_jet_backward(n, params, X, N, gY, gdY, grad_flat, ws, ws_bytes, (hipStream_t)stream);
}

int32_t pinn_jet_backward_kernel(const pinn_desc* desc, int64_t N, int32_t with_gdY, int32_t* kernel) {
  Net n; int rc = make_net(desc, &n); if (rc) return rc;
  if (!kernel || N < 0) { set_error("bad arguments"); return PINN_ERR_INVALID; }
  if (!with_gdY) { n.k = 0; n.K1 = 1; }      // as pinn_jet_backward with gdY == NULL: the plain network
  const int e = pick_jet_backward_engine(desc, n, &rc); if (rc) return rc;
  *kernel = e == PINN_ENGINE_FUSED ? fused_jet_backward_kernel(n, N) : PINN_ENGINE_GENERIC;
  return PINN_OK;
}

static int32_t residual_impl(const pinn_desc* desc, const pinn_residual_spec* spec, const float* term_scale,
                             const float* params, const float* X, int64_t N, float* term_sums, float* grad_flat,
                             void* ws, int64_t ws_bytes, void* stream, bool want_grad) {
  Net n; int rc = make_net(desc, &n); if (rc) return rc;
  LossReq rq; rc = build_request(n, spec, N, N, 0, 0, nullptr, &rq); if (rc) return rc;
  if (!params || (!X && N > 0) || N < 0 || !term_sums || (want_grad && (!grad_flat || !term_scale))) {
    set_error("NULL pointer argument"); return PINN_ERR_INVALID;
  }
  rq.scale = term_scale; rq.sums = term_sums; rq.grad = want_grad ? grad_flat : nullptr;
  if (N == 0) { (void)hipMemsetAsync(term_sums, 0, rq.n_terms * sizeof(float), (hipStream_t)stream); return PINN_OK; }
  return run_loss(desc, n, want_grad, rq, params, X, N, ws, ws_bytes, stream);
}

int32_t pinn_residual_loss(const pinn_desc* desc, const pinn_residual_spec* spec, const float* params,
                           const float* X, int64_t N, float* term_sums, void* ws, int64_t ws_bytes, void* stream) {
  return residual_impl(desc, spec, nullptr, params, X, N, term_sums, nullptr, ws, ws_bytes, stream, false);
}

int32_t pinn_residual_loss_grad(const pinn_desc* desc, const pinn_residual_spec* spec, const float* term_scale,
                                const float* params, const float* X, int64_t N, float* term_sums,
                                float* grad_flat, void* ws, int64_t ws_bytes, void* stream) {
  return residual_impl(desc, spec, term_scale, params, X, N, term_sums, grad_flat, ws, ws_bytes, stream, true);
}

int32_t pinn_mse_loss_grad(const pinn_desc* desc, const float* params, const float* X, const float* T, int64_t N,
                           int32_t n_cols, const int32_t* out_col, const float* col_scale, float* col_sums,
                           float* grad_flat, void* ws, int64_t ws_bytes, void* stream) {
  Net n; int rc = make_net(desc, &n); if (rc) return rc;
  if (!params || ((!X || !T) && N > 0) || N < 0 || !out_col || !col_sums || (grad_flat && !col_scale)) {
    set_error("NULL pointer argument"); return PINN_ERR_INVALID;
  }
  if (n_cols < 1 || n_cols > PINN_MAX_ROLES) { set_error("n_cols=%d outside 1..%d", n_cols, PINN_MAX_ROLES); return PINN_ERR_INVALID; }
  LossReq rq; memset(&rq, 0, sizeof(rq));
  rq.kind = 1; rq.n_split = -1; rq.T = T; rq.n_cols = n_cols; rq.mse_scale = col_scale; rq.mse_sums = col_sums; rq.grad = grad_flat;
  rc = set_out_cols(n, n_cols, out_col, &rq); if (rc) return rc;
  if (N == 0) { (void)hipMemsetAsync(col_sums, 0, n_cols * sizeof(float), (hipStream_t)stream); return PINN_OK; }
  n.k = 0; n.K1 = 1;  // the fidelity term needs no input derivatives
  return run_loss(desc, n, grad_flat != nullptr, rq, params, X, N, ws, ws_bytes, stream);
}

static int32_t residual_mse_impl(int64_t n_split, const pinn_desc* desc, const pinn_residual_spec* spec, const float* term_scale,
                                    const float* T, int32_t n_cols, const int32_t* out_col, const float* col_scale,
                                    const float* params, const float* X, int64_t N, float* term_sums,
                                    float* col_sums, float* grad_flat, void* ws, int64_t ws_bytes, void* stream) {
  Net n; int rc = make_net(desc, &n); if (rc) return rc;
  LossReq rq; rc = build_request(n, spec, N, n_split, 1, n_cols, out_col, &rq); if (rc) return rc;
  if (!params || ((!X || (!T && n_split != N)) && N > 0) || N < 0 || !term_sums || !col_sums || !out_col || !grad_flat || !term_scale ||
      !col_scale) {
    set_error("NULL pointer argument"); return PINN_ERR_INVALID;
  }
  rq.scale = term_scale; rq.sums = term_sums;
  rq.T = T; rq.mse_scale = col_scale; rq.mse_sums = col_sums; rq.grad = grad_flat;
  if (N == 0) {
    (void)hipMemsetAsync(term_sums, 0, rq.n_terms * sizeof(float), (hipStream_t)stream);
    (void)hipMemsetAsync(col_sums, 0, n_cols * sizeof(float), (hipStream_t)stream);
    return PINN_OK;
  }
  // no fidelity points: the residual-only pass (T may be NULL)
  if (rq.kind == 0) (void)hipMemsetAsync(col_sums, 0, n_cols * sizeof(float), (hipStream_t)stream);
  return run_loss(desc, n, true, rq, params, X, N, ws, ws_bytes, stream);
}

int32_t pinn_residual_mse_loss_grad(const pinn_desc* desc, const pinn_residual_spec* spec, const float* term_scale,
                                    const float* T, int32_t n_cols, const int32_t* out_col, const float* col_scale,
                                    const float* params, const float* X, int64_t N, float* term_sums,
                                    float* col_sums, float* grad_flat, void* ws, int64_t ws_bytes, void* stream) {
  return residual_mse_impl(-1, desc, spec, term_scale, T, n_cols, out_col, col_scale, params, X, N, term_sums, col_sums,
                           grad_flat, ws, ws_bytes, stream);
}

int32_t pinn_residual_mse_split_loss_grad(const pinn_desc* desc, const pinn_residual_spec* spec, const float* term_scale,
                                          const float* T, int32_t n_cols, const int32_t* out_col, const float* col_scale,
                                          const float* params, const float* X, int64_t N, int64_t n_res,
                                          float* term_sums, float* col_sums, float* grad_flat, void* ws,
                                          int64_t ws_bytes, void* stream) {
  if (n_res < 0) { set_error("n_res must be >= 0"); return PINN_ERR_INVALID; }
  return residual_mse_impl(n_res, desc, spec, term_scale, T, n_cols, out_col, col_scale, params, X, N, term_sums,
                           col_sums, grad_flat, ws, ws_bytes, stream);
}

int32_t pinn_adam_step(float* params, const float* grad, float* m, float* v, int64_t P, int64_t step, double lr,
                       double beta1, double beta2, double eps, void* stream) {
  if (!params || !grad || !m || !v || P < 0 || step < 1) { set_error("bad arguments"); return PINN_ERR_INVALID; }
  if (P == 0) return PINN_OK;
  hipLaunchKernelGGL(k_adam, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, params, grad, m,
                     v, P, adam_scalars(lr, beta1, beta2, eps, step));
  return check_launch("adam");
}

int32_t pinn_loss_grad_adam_step(const pinn_desc* desc, const pinn_residual_spec* spec, const float* term_scale,
                                 const float* T, int32_t n_cols, const int32_t* out_col, const float* col_scale,
                                 float* params, const float* X, int64_t N, int64_t n_res, float* term_sums,
                                 float* col_sums, float* grad_flat, const pinn_adam_state* adam, void* ws,
                                 int64_t ws_bytes, void* stream) {
  Net n; int rc = make_net(desc, &n); if (rc) return rc;
  if (!spec || !adam) { set_error("NULL pointer argument"); return PINN_ERR_INVALID; }
  LossReq rq; rc = build_request(n, spec, N, n_res, 0, n_cols, out_col, &rq); if (rc) return rc;
  if (!params || !X || N < 1 || !term_sums || !term_scale || !grad_flat || !adam->m || !adam->v || adam->step < 1) {
    set_error("bad arguments"); return PINN_ERR_INVALID;
  }
  if (n_cols > 0 && (!out_col || !col_scale || !col_sums || (!T && n_res != N))) { set_error("NULL pointer argument"); return PINN_ERR_INVALID; }
  rq.scale = term_scale; rq.sums = term_sums;
  rq.T = T; rq.mse_scale = col_scale; rq.mse_sums = col_sums; rq.grad = grad_flat;
  int e = pick_engine(desc, n, true, &rc);
  if (int rcc = corrected_engine(desc, n, rq, &e, rc)) return rcc;
  if (rc) return rc;
  if (e != PINN_ENGINE_FUSED || !fused_supports_adam(n, rq, N)) {
    set_error("pinn_loss_grad_adam_step: needs a one-pass request on the fused engine (use the loss call + pinn_adam_step)");
    return PINN_ERR_UNSUPPORTED;
  }
  AdamReq a; rc = adam_req(adam, params, &a); if (rc) return rc;
  rq.adam = &a;
  if (rq.kind == 0 && n_cols > 0) (void)hipMemsetAsync(col_sums, 0, n_cols * sizeof(float), (hipStream_t)stream);
  return fused_loss(n, rq, params, X, N, ws, ws_bytes, (hipStream_t)stream);
}

int32_t pinn_adam_loop(const pinn_desc* desc, const pinn_residual_spec* spec, const float* term_scale, const float* T,
                       int32_t n_cols, const int32_t* out_col, const float* col_scale, float* params, const float* X,
                       int64_t N, int64_t n_res, float* term_sums, float* col_sums, float* grad_flat,
                       const pinn_adam_state* adam, int32_t n_iters, const double* lr, void* ws, int64_t ws_bytes,
                       void* stream) {
  if (!adam || !lr || n_iters < 0) { set_error("bad arguments"); return PINN_ERR_INVALID; }
  for (int32_t i = 0; i < n_iters; ++i) {
    const pinn_adam_state st = adam_state_at(adam, i, lr, adam->n_loss_rows);
    const int32_t rc = pinn_loss_grad_adam_step(desc, spec, term_scale, T, n_cols, out_col, col_scale, params, X, N, n_res,
                                                term_sums, col_sums, grad_flat, &st, ws, ws_bytes, stream);
    if (rc) return rc;      // (unsupported requests are refused by the first iteration, before anything is launched)
  }
  return PINN_OK;
}

// ---- ensembles (pinn_hip.h; kernels: fused_kernel.h k_fused_ens, pinn_fused.hip) ------------------------------------------
// What the query, the plan and the calls share: the descriptor's network, M, and the refusals the descriptor alone decides.
// Pure host logic.
static int ensemble_net(const char* who, const pinn_desc* desc, int32_t M, Net* n) {
  int rc = make_net(desc, n); if (rc) return rc;
  if (M < 1 || M > PINN_ENSEMBLE_MAX_MEMBERS) {
    set_error("%s: M = %d outside 1..%d", who, M, PINN_ENSEMBLE_MAX_MEMBERS); return PINN_ERR_INVALID;
  }
  const int asked = asked_engine(desc);
  if (asked == PINN_ENGINE_GENERIC || asked == PINN_ENGINE_WIDE) {
    set_error("%s: engine %s has no ensemble kernel (use engine AUTO, FUSED or FUSED_TILE)", who,
              asked == PINN_ENGINE_GENERIC ? "GENERIC" : "WIDE");
    return PINN_ERR_UNSUPPORTED;
  }
  LossReq none; memset(&none, 0, sizeof(none)); none.kind = 1;      // (no spec, no split: the descriptor's part of the rule)
  if (const char* why = fused_ensemble_refusal(*n, none)) { set_error("%s: %s", who, why); return PINN_ERR_UNSUPPORTED; }
  return PINN_OK;
}

int32_t pinn_ensemble_query_workspace(const pinn_desc* desc, int32_t M, int64_t N, int64_t* bytes) {
  Net n; int rc = ensemble_net("pinn_ensemble_query_workspace", desc, M, &n); if (rc) return rc;
  if (!bytes || N < 1) { set_error("pinn_ensemble_query_workspace: bytes is NULL or N < 1"); return PINN_ERR_INVALID; }
  fused_ensemble_plan(n, M, N, nullptr, nullptr, bytes);
  return PINN_OK;
}

int32_t pinn_ensemble_plan(const pinn_desc* desc, int32_t M, int64_t N, int32_t* gx, int32_t* copy_in_lds) {
  Net n; int rc = ensemble_net("pinn_ensemble_plan", desc, M, &n); if (rc) return rc;
  if (!gx || !copy_in_lds || N < 1) { set_error("pinn_ensemble_plan: NULL pointer argument or N < 1"); return PINN_ERR_INVALID; }
  int g = 0, c = 0;
  fused_ensemble_plan(n, M, N, &g, &c, nullptr);
  *gx = g; *copy_in_lds = c;
  return PINN_OK;
}

// adam == nullptr: pinn_ensemble_loss_grad (grad +=); else the folded update (grad overwritten)
static int32_t ensemble_impl(const char* who, const pinn_desc* desc, const pinn_residual_spec* spec, int32_t M,
                             const float* term_scale, const float* T, int32_t n_cols, const int32_t* out_col,
                             const float* col_scale, const float* params, float* params_rw, const float* X, int64_t N,
                             int64_t n_res, int32_t flags, float* term_sums, float* col_sums, float* grad_flat,
                             const pinn_adam_state* adam, void* ws, int64_t ws_bytes, void* stream) {
  Net n; int rc = ensemble_net(who, desc, M, &n); if (rc) return rc;
  if (!spec) { set_error("%s: spec is NULL", who); return PINN_ERR_INVALID; }
  // (without out_col: no array is looked at before the refusals below; the columns follow the NULL checks)
  LossReq rq; rc = build_request(n, spec, N, n_res, 0, n_cols, nullptr, &rq); if (rc) return rc;
  if (N < 1) { set_error("%s: N = %lld, need at least one point", who, (long long)N); return PINN_ERR_INVALID; }
  if (flags & ~(PINN_ENSEMBLE_OWN_X | PINN_ENSEMBLE_OWN_T)) { set_error("%s: unknown flags 0x%x", who, flags); return PINN_ERR_INVALID; }
  rq.scale = term_scale; rq.sums = term_sums;
  rq.T = T; rq.mse_scale = col_scale; rq.mse_sums = col_sums; rq.grad = grad_flat;
  // the request's refusals (corrected radiation stress, the split request at width 64), before the pointers are looked at
  if (const char* why = fused_ensemble_refusal(n, rq)) { set_error("%s: %s", who, why); return PINN_ERR_UNSUPPORTED; }
  if (!params || !X || !term_sums || !term_scale || !grad_flat) { set_error("%s: NULL pointer argument", who); return PINN_ERR_INVALID; }
  if (n_cols > 0 && (!out_col || !col_scale || !col_sums || (!T && n_res != N))) { set_error("%s: NULL pointer argument", who); return PINN_ERR_INVALID; }
  rc = set_out_cols(n, n_cols, out_col, &rq); if (rc) return rc;
  AdamReq a;
  if (adam) {
    if (!adam->m || !adam->v || adam->step < 1) { set_error("%s: bad adam state", who); return PINN_ERR_INVALID; }
    rc = adam_req(adam, params_rw, &a); if (rc) return rc;
    rq.adam = &a;
  }
  int64_t need = 0;
  fused_ensemble_plan(n, M, N, nullptr, nullptr, &need);
  rc = check_workspace(ws, ws_bytes, need); if (rc) return rc;
  if (rq.kind == 0 && n_cols > 0) (void)hipMemsetAsync(col_sums, 0, (size_t)M * n_cols * sizeof(float), (hipStream_t)stream);
  return fused_ensemble_loss(n, rq, M, flags, params, X, N, ws, ws_bytes, (hipStream_t)stream);
}

int32_t pinn_ensemble_loss_grad(const pinn_desc* desc, const pinn_residual_spec* spec, int32_t M, const float* term_scale,
                                const float* T, int32_t n_cols, const int32_t* out_col, const float* col_scale,
                                const float* params, const float* X, int64_t N, int64_t n_res, int32_t flags,
                                float* term_sums, float* col_sums, float* grad_flat, void* ws, int64_t ws_bytes, void* stream) {
  return ensemble_impl("pinn_ensemble_loss_grad", desc, spec, M, term_scale, T, n_cols, out_col, col_scale, params, nullptr, X,
                       N, n_res, flags, term_sums, col_sums, grad_flat, nullptr, ws, ws_bytes, stream);
}

int32_t pinn_ensemble_adam_step(const pinn_desc* desc, const pinn_residual_spec* spec, int32_t M, const float* term_scale,
                                const float* T, int32_t n_cols, const int32_t* out_col, const float* col_scale, float* params,
                                const float* X, int64_t N, int64_t n_res, int32_t flags, float* term_sums, float* col_sums,
                                float* grad_flat, const pinn_adam_state* adam, void* ws, int64_t ws_bytes, void* stream) {
  if (!adam) { set_error("pinn_ensemble_adam_step: adam is NULL"); return PINN_ERR_INVALID; }
  return ensemble_impl("pinn_ensemble_adam_step", desc, spec, M, term_scale, T, n_cols, out_col, col_scale, params, params, X, N,
                       n_res, flags, term_sums, col_sums, grad_flat, adam, ws, ws_bytes, stream);
}

int32_t pinn_ensemble_adam_loop(const pinn_desc* desc, const pinn_residual_spec* spec, int32_t M, const float* term_scale,
                                const float* T, int32_t n_cols, const int32_t* out_col, const float* col_scale, float* params,
                                const float* X, int64_t N, int64_t n_res, int32_t flags, float* term_sums, float* col_sums,
                                float* grad_flat, const pinn_adam_state* adam, int32_t n_iters, const double* lr, void* ws,
                                int64_t ws_bytes, void* stream) {
  if (!adam || !lr || n_iters < 0) { set_error("pinn_ensemble_adam_loop: bad arguments"); return PINN_ERR_INVALID; }
  for (int32_t i = 0; i < n_iters; ++i) {
    const pinn_adam_state st = adam_state_at(adam, i, lr, (int64_t)M * adam->n_loss_rows);
    const int32_t rc = pinn_ensemble_adam_step(desc, spec, M, term_scale, T, n_cols, out_col, col_scale, params, X, N, n_res,
                                               flags, term_sums, col_sums, grad_flat, &st, ws, ws_bytes, stream);
    if (rc) return rc;      // (refusals come from the first iteration, before anything is launched)
  }
  return PINN_OK;
}

// ---- device-resident L-BFGS (pinn_hip.h; kernels: pinn_lbfgs_loop.hip, line search: lbfgs_line_search.h) ---------------
int32_t pinn_lbfgs_ls_init(pinn_ls_state* st, double f0, double gtd0, double t0, double d_norm, int32_t max_ls) {
  if (!st) { set_error("pinn_lbfgs_ls_init: state is NULL"); return PINN_ERR_INVALID; }
  return ls_init(st, f0, gtd0, t0, d_norm, max_ls);
}

int32_t pinn_lbfgs_ls_step(pinn_ls_state* st, double f_new, double gtd_new) {
  if (!st) { set_error("pinn_lbfgs_ls_step: state is NULL"); return PINN_ERR_INVALID; }
  if (st->phase < 0 || st->phase > 2 || st->g_slot_for_new < 1 || st->g_slot_for_new >= PINN_LS_POOL_ROWS) {
    set_error("pinn_lbfgs_ls_step: the state was not armed by pinn_lbfgs_ls_init"); return PINN_ERR_INVALID;
  }
  return ls_step(st, f_new, gtd_new);
}

// what the query, the init and the loop share: the descriptor's network, refused with dropout
static int lbfgs_loop_net(const char* who, const pinn_desc* desc, Net* n) {
  int rc = make_net(desc, n); if (rc) return rc;
  if (n->drop_p > 0.f) {
    set_error("%s: dropout_p > 0 is not supported (a seed per forward pass has no place in a fixed schedule of slots)", who);
    return PINN_ERR_UNSUPPORTED;
  }
  return PINN_OK;
}
static int lbfgs_history_ok(const char* who, int32_t m) {
  if (m < 1 || m > LBL_MAX_M) { set_error("%s: history_size = %d outside 1..%d", who, m, LBL_MAX_M); return PINN_ERR_INVALID; }
  return PINN_OK;
}

int32_t pinn_query_lbfgs_loop(const pinn_desc* desc, int64_t N, int32_t history_size, int64_t* ws_bytes, int64_t* state_bytes) {
  Net n; int rc = lbfgs_loop_net("pinn_query_lbfgs_loop", desc, &n); if (rc) return rc;
  rc = lbfgs_history_ok("pinn_query_lbfgs_loop", history_size); if (rc) return rc;
  if (!ws_bytes || !state_bytes || N < 1) { set_error("pinn_query_lbfgs_loop: bad arguments"); return PINN_ERR_INVALID; }
  rc = pinn_query_workspace(desc, N, ws_bytes); if (rc) return rc;
  *state_bytes = lbl_layout(n.n_params(), history_size).total;
  return PINN_OK;
}

int32_t pinn_lbfgs_loop_init(void* state, int64_t state_bytes, int64_t P, const pinn_lbfgs_opts* opts, void* stream) {
  if (!state || !opts || P < 1) { set_error("pinn_lbfgs_loop_init: NULL pointer argument or P < 1"); return PINN_ERR_INVALID; }
  int rc = lbfgs_history_ok("pinn_lbfgs_loop_init", opts->history_size); if (rc) return rc;
  if (opts->max_iter < 0 || opts->max_eval < 1 || !(opts->lr > 0.0)) {
    set_error("pinn_lbfgs_loop_init: max_iter = %d, max_eval = %d, lr = %g", opts->max_iter, opts->max_eval, opts->lr);
    return PINN_ERR_INVALID;
  }
  const int64_t need = lbl_layout(P, opts->history_size).total;
  if (state_bytes < need) {
    set_error("pinn_lbfgs_loop_init: state too small: need %lld bytes, got %lld", (long long)need, (long long)state_bytes);
    return PINN_ERR_WORKSPACE;
  }
  return lbl_init(state, state_bytes, P, *opts, (hipStream_t)stream);
}

int32_t pinn_lbfgs_loop(const pinn_desc* desc, const pinn_residual_spec* spec, const float* term_scale, const float* T,
                        int32_t n_cols, const int32_t* out_col, const float* col_scale, float* params, const float* X,
                        int64_t N, int64_t n_res, int32_t n_loss_rows, const float* loss_rows, int32_t total_row,
                        void* state, int64_t state_bytes, int32_t n_slots, double* trace,
                        void* ws, int64_t ws_bytes, void* stream) {
  Net n; int rc = lbfgs_loop_net("pinn_lbfgs_loop", desc, &n); if (rc) return rc;
  if (!spec) { set_error("pinn_lbfgs_loop: NULL pointer argument"); return PINN_ERR_INVALID; }
  LossReq rq; rc = build_request(n, spec, N, n_res, 0, n_cols, out_col, &rq); if (rc) return rc;
  if (!params || !X || N < 1 || !term_scale || !state || !loss_rows) { set_error("pinn_lbfgs_loop: NULL pointer argument or N < 1"); return PINN_ERR_INVALID; }
  if (n_slots < 0) { set_error("pinn_lbfgs_loop: n_slots = %d", n_slots); return PINN_ERR_INVALID; }
  if (n_cols > 0 && (!out_col || !col_scale || (!T && n_res != N))) { set_error("pinn_lbfgs_loop: NULL pointer argument"); return PINN_ERR_INVALID; }
  if (n_loss_rows < 1 || n_loss_rows > 8 || total_row < 0 || total_row >= n_loss_rows) {
    set_error("pinn_lbfgs_loop: n_loss_rows = %d outside 1..8 or total_row = %d outside it", n_loss_rows, total_row);
    return PINN_ERR_INVALID;
  }
  const int64_t P = n.n_params();
  const int64_t need = lbl_layout(P, 1).total;      // (the history's share was checked by pinn_lbfgs_loop_init, which knows m)
  if (state_bytes < need) {
    set_error("pinn_lbfgs_loop: state too small: need at least %lld bytes, got %lld", (long long)need, (long long)state_bytes);
    return PINN_ERR_WORKSPACE;
  }
  const LblPtrs p = lbl_ptrs(state, params, P, n_cols);
  rq.scale = term_scale;
  rq.T = T; rq.mse_scale = col_scale; rq.mse_sums = p.csums; rq.sums = p.tsums; rq.grad = p.gnew;
  {   // the refusals of the loss request itself, before anything is launched
    int e = pick_engine(desc, n, true, &rc);
    if (int rcc = corrected_engine(desc, n, rq, &e, rc)) return rcc;
    if (rc) return rc;
    const int64_t ws_need = engine_workspace_bytes(e, n, N);
    if (ws_need < 0) { set_error("network not supported"); return PINN_ERR_UNSUPPORTED; }
    rc = check_workspace(ws, ws_bytes, ws_need); if (rc) return rc;
  }
  const hipStream_t s = (hipStream_t)stream;
  for (int32_t i = 0; i < n_slots; ++i) {
    rc = lbl_before_pass(p, n_cols, rq.n_terms, s); if (rc) return rc;
    rc = run_loss(desc, n, true, rq, p.xt, X, N, ws, ws_bytes, stream); if (rc) return rc;
    rc = lbl_after_pass(p, n_cols, rq.n_terms, n_loss_rows, loss_rows, total_row,
                        trace ? trace + (int64_t)i * PINN_LBFGS_TRACE_COLS : nullptr, s);
    if (rc) return rc;
  }
  return PINN_OK;
}

// ---- the ensemble's device-resident L-BFGS (pinn_hip.h; kernels: pinn_lbfgs_ens.hip, the pass: fused_ensemble_loss) ----------
int32_t pinn_ensemble_query_lbfgs_loop(const pinn_desc* desc, int32_t M, int64_t N, int32_t history_size, int64_t* ws_bytes,
                                       int64_t* state_bytes) {
  const char* who = "pinn_ensemble_query_lbfgs_loop";
  Net n; int rc = ensemble_net(who, desc, M, &n); if (rc) return rc;
  rc = lbfgs_history_ok(who, history_size); if (rc) return rc;
  if (!ws_bytes || !state_bytes || N < 1) { set_error("%s: bad arguments", who); return PINN_ERR_INVALID; }
  fused_ensemble_plan(n, M, N, nullptr, nullptr, ws_bytes);
  *state_bytes = lbe_layout(M, n.n_params(), history_size).total;
  return PINN_OK;
}

int32_t pinn_ensemble_lbfgs_loop_init(void* state, int64_t state_bytes, int32_t M, int64_t P, const pinn_lbfgs_opts* opts,
                                      void* stream) {
  const char* who = "pinn_ensemble_lbfgs_loop_init";
  if (!state || !opts || P < 1) { set_error("%s: NULL pointer argument or P < 1", who); return PINN_ERR_INVALID; }
  if (M < 1 || M > PINN_ENSEMBLE_MAX_MEMBERS) { set_error("%s: M = %d outside 1..%d", who, M, PINN_ENSEMBLE_MAX_MEMBERS); return PINN_ERR_INVALID; }
  int rc = lbfgs_history_ok(who, opts->history_size); if (rc) return rc;
  if (opts->max_iter < 0 || opts->max_eval < 1 || !(opts->lr > 0.0)) {
    set_error("%s: max_iter = %d, max_eval = %d, lr = %g", who, opts->max_iter, opts->max_eval, opts->lr);
    return PINN_ERR_INVALID;
  }
  const int64_t need = lbe_layout(M, P, opts->history_size).total;
  if (state_bytes < need) {
    set_error("%s: state too small: need %lld bytes, got %lld", who, (long long)need, (long long)state_bytes);
    return PINN_ERR_WORKSPACE;
  }
  return lbe_init(state, M, P, *opts, (hipStream_t)stream);
}

int32_t pinn_ensemble_lbfgs_loop(const pinn_desc* desc, const pinn_residual_spec* spec, int32_t M, const float* term_scale,
                                 const float* T, int32_t n_cols, const int32_t* out_col, const float* col_scale, float* params,
                                 const float* X, int64_t N, int64_t n_res, int32_t flags, int32_t n_loss_rows,
                                 const float* loss_rows, int32_t total_row, int32_t history_size, void* state,
                                 int64_t state_bytes, int32_t n_slots, double* trace, void* ws, int64_t ws_bytes, void* stream) {
  const char* who = "pinn_ensemble_lbfgs_loop";
  Net n; int rc = ensemble_net(who, desc, M, &n); if (rc) return rc;
  rc = lbfgs_history_ok(who, history_size); if (rc) return rc;
  if (n_slots < 0) { set_error("%s: n_slots = %d", who, n_slots); return PINN_ERR_INVALID; }
  if (!spec) { set_error("%s: spec is NULL", who); return PINN_ERR_INVALID; }
  // (without out_col: no array is looked at before the refusals below; the columns follow the NULL checks)
  LossReq rq; rc = build_request(n, spec, N, n_res, 0, n_cols, nullptr, &rq); if (rc) return rc;
  if (N < 1) { set_error("%s: N = %lld, need at least one point", who, (long long)N); return PINN_ERR_INVALID; }
  if (flags & ~(PINN_ENSEMBLE_OWN_X | PINN_ENSEMBLE_OWN_T)) { set_error("%s: unknown flags 0x%x", who, flags); return PINN_ERR_INVALID; }
  if (const char* why = fused_ensemble_refusal(n, rq)) { set_error("%s: %s", who, why); return PINN_ERR_UNSUPPORTED; }
  if (n_loss_rows < 1 || n_loss_rows > 8 || total_row < 0 || total_row >= n_loss_rows) {
    set_error("%s: n_loss_rows = %d outside 1..8 or total_row = %d outside it", who, n_loss_rows, total_row);
    return PINN_ERR_INVALID;
  }
  if (!params || !X || !term_scale || !state || !loss_rows) { set_error("%s: NULL pointer argument", who); return PINN_ERR_INVALID; }
  if (n_cols > 0 && (!out_col || !col_scale || (!T && n_res != N))) { set_error("%s: NULL pointer argument", who); return PINN_ERR_INVALID; }
  rc = set_out_cols(n, n_cols, out_col, &rq); if (rc) return rc;
  const int64_t P = n.n_params();
  const int64_t need = lbe_layout(M, P, history_size).total;
  if (state_bytes < need) {
    set_error("%s: state too small: need %lld bytes, got %lld", who, (long long)need, (long long)state_bytes);
    return PINN_ERR_WORKSPACE;
  }
  int64_t ws_need = 0;
  fused_ensemble_plan(n, M, N, nullptr, nullptr, &ws_need);
  rc = check_workspace(ws, ws_bytes, ws_need); if (rc) return rc;
  const LbePtrs e = lbe_ptrs(state, params, M, P, history_size, n_cols, rq.n_terms);
  rq.scale = term_scale;
  rq.T = T; rq.mse_scale = col_scale; rq.mse_sums = lbe_csums(e); rq.sums = lbe_tsums(e); rq.grad = lbe_gnew(e);
  const hipStream_t s = (hipStream_t)stream;
  for (int32_t i = 0; i < n_slots; ++i) {
    rc = lbe_before_pass(e, s); if (rc) return rc;
    rc = fused_ensemble_loss(n, rq, M, flags, lbe_xt(e), X, N, ws, ws_bytes, s); if (rc) return rc;
    rc = lbe_after_pass(e, n_loss_rows, loss_rows, total_row,
                        trace ? trace + (int64_t)i * M * PINN_LBFGS_TRACE_COLS : nullptr, s);
    if (rc) return rc;
  }
  return PINN_OK;
}

// ---- per-point residual fields -------------------------------------------------------------------------------------
// Two paths. The fused tile kernel's field instances (one launch, nothing staged) where fused_tile_refusal(TILE_FIELD) has none; for
// every other request the descriptor's own pinn_forward_jet into a staging area, FIELDS_CHUNK points at a time (fixed:
// the staging stays bounded however large the pool), followed by the point-wise kernel of pinn_fields.hip.
// AUTO: the first where it applies, else the second.  FUSED (and sub-values): the first or refused, as pinn_jet_backward.
// GENERIC / WIDE: the second, on that engine.
static constexpr int64_t FIELDS_CHUNK = 1 << 16;

struct FieldsPlan {
  bool fused;                            // the tile kernel's field instances
  int64_t chunk, y_off, dy_off, in_off, inner_bytes, total;   // staged path: layout of the workspace
};

// validation shared by the query and the call (no HIP call before it has passed)
static int fields_plan(const pinn_desc* desc, const pinn_residual_spec* spec, int64_t N, Net* n, pinn_residual_spec* nspec,
                       FieldsPlan* pl) {
  int rc = make_net(desc, n); if (rc) return rc;
  rc = check_spec(*n, spec, nspec); if (rc) return rc;
  const bool corrected = is_pe_closure(nspec->residual_id), wave = nspec->residual_id == RES_PE_WAVE;
  rc = check_k("pinn_residual_fields", *n, spec, wave ? " (wave closure)" : corrected ? " (corrected radiation stress)" : ""); if (rc) return rc;
  if (N < 1) { set_error("pinn_residual_fields: N = %lld, need at least one point", (long long)N); return PINN_ERR_INVALID; }
  const int asked = asked_engine(desc);
  const char* why = fused_tile_refusal(TILE_FIELD, *n);
  // (the corrected radiation stress: the tile kernel's EPI_FIELD_PEC instances, tanh only; everything else is staged)
  const char* why_pec = corrected ? fused_corrected_refusal(*n) : nullptr;
  if (asked == PINN_ENGINE_FUSED && !why && why_pec) {
    set_error("pinn_residual_fields on the fused engine: %s %s; engine AUTO "
              "runs this request through the forward jet", pe_closure_name(wave), why_pec);
    return PINN_ERR_UNSUPPORTED;
  }
  const bool fused_ok = !why && !why_pec;
  if (asked == PINN_ENGINE_FUSED && why) {
    set_error("pinn_residual_fields on the fused engine: %s (width %d, d_in %d, d_out %d, k %d, hidden layers %d); "
              "engine AUTO runs this request through the forward jet", why, n->W, n->d_in, n->d_out, n->k, n->L);
    return PINN_ERR_UNSUPPORTED;
  }
  pl->fused = fused_ok && (asked == PINN_ENGINE_AUTO || asked == PINN_ENGINE_FUSED);
  if (pl->fused) {
    pl->chunk = N; pl->y_off = pl->dy_off = pl->in_off = 0; pl->inner_bytes = 0;
    pl->total = fused_fields_workspace_bytes(*n);
    return PINN_OK;
  }
  const int e = pick_engine(desc, *n, false, &rc); if (rc) return rc;   // the engine pinn_forward_jet will run on
  pl->chunk = N < FIELDS_CHUNK ? N : FIELDS_CHUNK;
  pl->inner_bytes = engine_workspace_bytes(e, *n, pl->chunk);
  if (pl->inner_bytes < 0) { set_error("network not supported"); return PINN_ERR_UNSUPPORTED; }
  int64_t off = 0;
  pl->y_off = off; off += align256(pl->chunk * n->d_out * 4);
  pl->dy_off = off; off += align256((int64_t)n->k * pl->chunk * n->d_out * 4);
  pl->in_off = off; off += align256(pl->inner_bytes);
  pl->total = off;
  return PINN_OK;
}

int32_t pinn_query_fields_workspace(const pinn_desc* desc, const pinn_residual_spec* spec, int64_t N, int64_t* bytes) {
  Net n; pinn_residual_spec nspec; FieldsPlan pl;
  int rc = fields_plan(desc, spec, N, &n, &nspec, &pl); if (rc) return rc;
  if (!bytes) { set_error("bytes is NULL"); return PINN_ERR_INVALID; }
  *bytes = pl.total;
  return PINN_OK;
}

int32_t pinn_residual_fields(const pinn_desc* desc, const pinn_residual_spec* spec, const float* params, const float* X,
                             int64_t N, float* fields, void* ws, int64_t ws_bytes, void* stream) {
  Net n; pinn_residual_spec nspec; FieldsPlan pl;
  int rc = fields_plan(desc, spec, N, &n, &nspec, &pl); if (rc) return rc;
  if (!params || !X || !fields) { set_error("NULL pointer argument"); return PINN_ERR_INVALID; }
  rc = check_workspace(ws, ws_bytes, pl.total); if (rc) return rc;
  const hipStream_t s = (hipStream_t)stream;
  if (pl.fused) return fused_residual_fields(n, nspec, params, X, N, fields, ws, ws_bytes, s);
  char* base = (char*)ws;
  float* Y = (float*)(base + pl.y_off);
  float* dY = (float*)(base + pl.dy_off);
  for (int64_t n0 = 0; n0 < N; n0 += pl.chunk) {
    const int64_t nc = N - n0 < pl.chunk ? N - n0 : pl.chunk;
    const float* Xc = X + n0 * n.d_in;
    rc = forward_impl(desc, params, Xc, nc, Y, dY, base + pl.in_off, pl.inner_bytes, stream, true); if (rc) return rc;
    rc = fields_from_jet(n, nspec, Xc, Y, dY, nc, n0, N, fields, s); if (rc) return rc;
  }
  return PINN_OK;
}

// ---- second-order jets (physics.py:6-15 applied twice; their parameter gradient, train.py:191) ----------------------
// Validation shared by the three jet2 entries; *mfma = which layer kernels run.  GENERIC: the VALU kernels, any shape.
// FUSED (and its sub-values): the MFMA kernels, fp32 networks at most 64 wide without dropout, refused otherwise.
// AUTO: MFMA where it applies, else the generic kernels (dropout, wider networks).
static int jet2_net(const pinn_desc* desc, Net* n, bool* mfma) {
  int rc = make_net(desc, n); if (rc) return rc;
  if (n->k < 1) { set_error("jet2 needs k >= 1 differentiated inputs (k = %d)", n->k); return PINN_ERR_INVALID; }
  if (n->act == PINN_ACT_SIN_TANH) {
    set_error("the second-order entries (jet2, residual2) serve activation 0 (tanh) and 1 (LeakyReLU) only: the sine first "
              "layer (activation 2) has no second-order kernel on any engine");
    return PINN_ERR_UNSUPPORTED;
  }
  if (n->prec != PINN_PREC_F32) { set_error("jet2 is implemented in fp32 only (precision bf16 refused)"); return PINN_ERR_UNSUPPORTED; }
  const int asked = asked_engine(desc);
  if (asked == PINN_ENGINE_WIDE) { set_error("jet2 does not run on the wide engine: use engine AUTO, FUSED or GENERIC"); return PINN_ERR_UNSUPPORTED; }
  const bool ok = jet2_mfma_supports(*n);
  if (asked == PINN_ENGINE_FUSED && !ok) {
    if (n->drop_p > 0.f)
      set_error("jet2 with dropout_p > 0 is not served by the MFMA (fused) path: use engine AUTO or GENERIC");
    else
      set_error("the MFMA (fused) jet2 path serves layers at most 64 wide (d_in %d, width %d, d_out %d): use engine AUTO or GENERIC",
                n->d_in, n->W, n->d_out);
    return PINN_ERR_UNSUPPORTED;
  }
  *mfma = ok && asked != PINN_ENGINE_GENERIC;
  return PINN_OK;
}

int32_t pinn_query_jet2_workspace(const pinn_desc* desc, int64_t N, int64_t* bytes) {
  Net n; bool mfma; int rc = jet2_net(desc, &n, &mfma); if (rc) return rc;
  if (!bytes || N < 0) { set_error("bad arguments"); return PINN_ERR_INVALID; }
  const int64_t b = jet2_workspace_bytes(n, N);
  if (b < 0) { set_error("too many layers for the jet2 kernels"); return PINN_ERR_UNSUPPORTED; }
  *bytes = b;
  return PINN_OK;
}

int32_t pinn_forward_jet2(const pinn_desc* desc, const float* params, const float* X, int64_t N, float* Y, float* dY,
                          float* d2Y, void* ws, int64_t ws_bytes, void* stream) {
  Net n; bool mfma; int rc = jet2_net(desc, &n, &mfma); if (rc) return rc;
  if (!params || (!X && N > 0) || N < 0 || (!d2Y && N > 0)) { set_error("NULL pointer argument"); return PINN_ERR_INVALID; }
  if (N == 0) return PINN_OK;
  return jet2_forward(n, mfma, params, X, N, Y, dY, d2Y, ws, ws_bytes, (hipStream_t)stream);
}

int32_t pinn_jet2_backward(const pinn_desc* desc, const float* params, const float* X, int64_t N, const float* gY,
                           const float* gdY, const float* gd2Y, float* grad_flat, void* ws, int64_t ws_bytes,
                           void* stream) {
  Net n; bool mfma; int rc = jet2_net(desc, &n, &mfma); if (rc) return rc;
  if (!params || (!X && N > 0) || N < 0 || !grad_flat) { set_error("NULL pointer argument"); return PINN_ERR_INVALID; }
  if (N == 0 || (!gY && !gdY && !gd2Y)) return PINN_OK;   // nothing to add
  return jet2_backward(n, mfma, params, X, N, gY, gdY, gd2Y, grad_flat, ws, ws_bytes, (hipStream_t)stream);
}

// ---- the lateral-mixing term nu * lap(U) on the second-order jets ------------------------------------------------------
// the three residuals with a momentum equation, on the host: the very functions k2_residual calls (residuals.h)
extern "C++" {
template <class B>
static void residual2_point(float nu, const float* v, const float* lap, const float* scale, float* fields, float* g,
                            float* glap) {
  typedef Residual2<B> R;
  float f[R::NF];
  const float l2[2] = {lap[0], lap[1]};
  point_jet<R>(v, g, [&](const float (&jet)[1 + R::ND][R::NR], float (&gj)[1 + R::ND][R::NR]) {
    if (!scale || !g || !glap) { R::fields(jet, l2, nu, f); return false; }
    float gl[2];
    R::template eval<true>(jet, l2, nu, scale, f, gj, gl);
    glap[0] = gl[0]; glap[1] = gl[1];
    return true;
  });
  for (int t = 0; t < R::NF; ++t) fields[t] = f[t];
}
}  // extern "C++"

static int check_nu(float nu) {
  if (!(nu >= 0.f) || !isfinite(nu)) { set_error("nu = %g: the eddy viscosity must be finite and >= 0", (double)nu); return PINN_ERR_INVALID; }
  return PINN_OK;
}

int32_t pinn_residual2_point(int32_t residual_id, int32_t flags, float nu, const float* v, const float lap[2],
                             const float* scale, float* fields, float* g, float glap[2]) {
  int rc = check_nu(nu); if (rc) return rc;
  if (!v || !lap || !fields) { set_error("NULL pointer argument"); return PINN_ERR_INVALID; }
  switch (residual_id) {
    case PINN_RES_NAVIER_STOKES: residual2_point<Res2NavierStokes>(nu, v, lap, scale, fields, g, glap); return PINN_OK;
    case PINN_RES_PHYSICS_EQUATION:
      if (flags & 2) { set_error("pinn_residual2_point: %s has no second-order form", pe_closure_name(true)); return PINN_ERR_UNSUPPORTED; }
      if (flags & 1) residual2_point<Res2PhysicsEquationCorrected>(nu, v, lap, scale, fields, g, glap);
      else residual2_point<Res2PhysicsEquation>(nu, v, lap, scale, fields, g, glap);
      return PINN_OK;
    case PINN_RES_CONTINUITY_FTEMP: case PINN_RES_CONTINUITY_ONLY:
      set_error("residual %d has no momentum equation: no second-order term", residual_id);
      return PINN_ERR_UNSUPPORTED;
    default: set_error("unknown residual_id %d", residual_id); return PINN_ERR_INVALID;
  }
}

// validation shared by the query and the call (no HIP call before it has passed)
static int residual2_plan(const pinn_desc* desc, const pinn_residual_spec* spec, Net* n, pinn_residual_spec* nspec, bool* mfma) {
  int rc = make_net(desc, n); if (rc) return rc;
  rc = check_spec(*n, spec, nspec); if (rc) return rc;
  if (is_wave_spec(spec)) {
    set_error("pinn_residual2_loss_grad: %s has no second-order form (nu together with the wave closure): use "
              "pinn_residual_loss_grad, or flags = 1 here", pe_closure_name(true));
    return PINN_ERR_UNSUPPORTED;
  }
  if (spec->residual_id == PINN_RES_CONTINUITY_FTEMP || spec->residual_id == PINN_RES_CONTINUITY_ONLY) {
    set_error("pinn_residual2_loss_grad: residual %d has no momentum equation: no second-order term", spec->residual_id);
    return PINN_ERR_UNSUPPORTED;
  }
  rc = check_k("pinn_residual2_loss_grad", *n, spec, ""); if (rc) return rc;
  return jet2_net(desc, n, mfma);
}

int32_t pinn_query_residual2_workspace(const pinn_desc* desc, const pinn_residual_spec* spec, int64_t N, int64_t* bytes) {
  Net n; pinn_residual_spec nspec; bool mfma;
  int rc = residual2_plan(desc, spec, &n, &nspec, &mfma); if (rc) return rc;
  if (!bytes || N < 0) { set_error("bad arguments"); return PINN_ERR_INVALID; }
  const int64_t b = residual2_workspace_bytes(n, N);
  if (b < 0) { set_error("too many layers for the jet2 kernels"); return PINN_ERR_UNSUPPORTED; }
  *bytes = b;
  return PINN_OK;
}

int32_t pinn_residual2_loss_grad(const pinn_desc* desc, const pinn_residual_spec* spec, float nu, const float* term_scale,
                                 const float* params, const float* X, int64_t N, float* term_sums, float* fields,
                                 float* grad_flat, void* ws, int64_t ws_bytes, void* stream) {
  Net n; pinn_residual_spec nspec; bool mfma;
  int rc = residual2_plan(desc, spec, &n, &nspec, &mfma); if (rc) return rc;
  rc = check_nu(nu); if (rc) return rc;
  if (!params || (!X && N > 0) || N < 0 || !term_sums || (grad_flat && !term_scale)) {
    set_error("NULL pointer argument"); return PINN_ERR_INVALID;
  }
  if (N == 0) { (void)hipMemsetAsync(term_sums, 0, residual_terms(spec->residual_id) * sizeof(float), (hipStream_t)stream); return PINN_OK; }
  return residual2_loss_grad(n, mfma, nspec, nu, term_scale, params, X, N, term_sums, fields, grad_flat, ws, ws_bytes,
                             (hipStream_t)stream);
}

// ---- runtime closure coefficients: gamma_b of Navier_Stokes, Cd of the plain physics_equation ---------------------------
// the two residuals with a coefficient, on the host: the very functions the kernels call (residuals.h)
extern "C++" {
template <class R>
static void residual_coef_point(const float* v, const float* coef, const float* scale, float* fields, float* g, float* gcoef) {
  point_jet<R>(v, g, [&](const float (&jet)[1 + R::ND][R::NR], float (&gj)[1 + R::ND][R::NR]) {
    float f[R::NF], sq[R::NT], gc[R::NC];
    R::fields(jet, coef, f);
    for (int t = 0; t < R::NF; ++t) fields[t] = f[t];
    if (!scale || !g || !gcoef) return false;
    R::template eval<true>(jet, coef, scale, gj, sq, gc);
    for (int j = 0; j < R::NC; ++j) gcoef[j] = gc[j];
    return true;
  });
}
}  // extern "C++"

// 0 = the residual has a coefficient form; else the refusal ("no coefficient" / "corrected" in the message) or INVALID
static bool is_corrected(int residual_id, int flags) { return residual_id == PINN_RES_PHYSICS_EQUATION && (flags & 1); }
static int coef_residual(const char* who, int residual_id, int flags) {
  if (!residual_info(residual_id)) { set_error("unknown residual_id %d", residual_id); return PINN_ERR_INVALID; }
  if (is_corrected(residual_id, flags)) {
    set_error("%s: %s has no coefficient form", who, pe_closure_name((flags & 2) != 0));
    return PINN_ERR_UNSUPPORTED;
  }
  if (residual_id != PINN_RES_NAVIER_STOKES && residual_id != PINN_RES_PHYSICS_EQUATION) {
    set_error("%s: residual %d has no closure: no coefficient", who, residual_id);
    return PINN_ERR_UNSUPPORTED;
  }
  return PINN_OK;
}

int32_t pinn_residual_coef_count(int32_t residual_id, int32_t flags, int32_t* n) {
  if (!n) { set_error("n is NULL"); return PINN_ERR_INVALID; }
  const int rc = coef_residual("pinn_residual_coef_count", residual_id, flags);
  if (rc == PINN_ERR_INVALID) return rc;
  *n = rc == PINN_OK ? 1 : 0;      // (a residual without a coefficient form is no error here: it has none)
  return PINN_OK;
}

int32_t pinn_residual_coef_default(int32_t residual_id, int32_t j, float* value) {
  if (!value) { set_error("value is NULL"); return PINN_ERR_INVALID; }
  int rc = coef_residual("pinn_residual_coef_default", residual_id, 0); if (rc) return rc;
  if (j != 0) { set_error("pinn_residual_coef_default: residual %d has 1 coefficient, j = %d", residual_id, j); return PINN_ERR_INVALID; }
  *value = residual_id == PINN_RES_NAVIER_STOKES ? ResNavierStokesCoef::DEFAULTS[0] : ResPhysicsEquationCoef::DEFAULTS[0];
  return PINN_OK;
}

int32_t pinn_residual_coef_point(int32_t residual_id, const float* v, const float* coef, const float* scale, float* fields,
                                 float* g, float* gcoef) {
  int rc = coef_residual("pinn_residual_coef_point", residual_id, 0); if (rc) return rc;
  if (!v || !coef || !fields) { set_error("NULL pointer argument"); return PINN_ERR_INVALID; }
  if (residual_id == PINN_RES_NAVIER_STOKES) residual_coef_point<ResNavierStokesCoef>(v, coef, scale, fields, g, gcoef);
  else residual_coef_point<ResPhysicsEquationCoef>(v, coef, scale, fields, g, gcoef);
  return PINN_OK;
}

// ---- the residual with coefficients or with point weights: the single entries and pinn_adam_loop_ext ----------------------
// The rules the three share, in the order of the header's tables, after the network and the spec have passed (no HIP call
// before a refusal).  What differs is passed in: the family (TILE_COEF refuses the residuals without a coefficient form,
// TILE_WEIGHTED the corrected radiation stress), whether k is checked before that refusal (the weighted entry's table) or
// after it, and whether the request may leave the tile kernel: the single entries run AUTO and GENERIC on the generic
// engine where the tile kernel has no instance, pinn_adam_loop_ext runs there or nowhere.
// *engine <- PINN_ENGINE_FUSED (the tile kernel's instances of the family) or PINN_ENGINE_GENERIC.
static int extra_rules(const char* who, int family, bool k_first, bool single, const pinn_desc* desc, const Net& n,
                       const pinn_residual_spec* spec, int* engine) {
  int rc = PINN_OK;
  if (k_first) { rc = check_k(who, n, spec, ""); if (rc) return rc; }
  if (family == TILE_COEF) { rc = coef_residual(who, spec->residual_id, spec->flags); if (rc) return rc; }
  else if (is_corrected(spec->residual_id, spec->flags)) {
    set_error("%s: %s has no point-weighted form", who, pe_closure_name((spec->flags & 2) != 0));
    return PINN_ERR_UNSUPPORTED;
  }
  if (!k_first) { rc = check_k(who, n, spec, ""); if (rc) return rc; }
  if (n.prec != PINN_PREC_F32) { set_error("%s is implemented in fp32 only (precision bf16 refused)", who); return PINN_ERR_UNSUPPORTED; }
  const int asked = asked_engine(desc);
  if (single && asked == PINN_ENGINE_WIDE) { set_error("%s does not run on the wide engine: use engine AUTO, FUSED or GENERIC", who); return PINN_ERR_UNSUPPORTED; }
  if (!single && (asked == PINN_ENGINE_GENERIC || asked == PINN_ENGINE_WIDE)) {
    set_error("%s runs on the fused tile kernel only (engine AUTO, FUSED or FUSED_TILE), not on engine %d: use the single "
              "entries and pinn_adam_step", who, desc->engine);
    return PINN_ERR_UNSUPPORTED;
  }
  const char* why = single ? fused_tile_refusal(family, n) : fused_adam_ext_refusal(n, family);
  if (why && (asked == PINN_ENGINE_FUSED || !single)) {
    set_error("%s%s: %s (width %d, d_in %d, d_out %d, k %d, activation %d, dropout_p %g); %s", who, single ? " on the fused engine" : "",
              why, n.W, n.d_in, n.d_out, n.k, n.act, (double)n.drop_p,
              single ? "engine AUTO or GENERIC runs this request on the generic engine" : "use the single entries and pinn_adam_step");
    return PINN_ERR_UNSUPPORTED;
  }
  *engine = (asked != PINN_ENGINE_GENERIC && !why) ? PINN_ENGINE_FUSED : PINN_ENGINE_GENERIC;
  return PINN_OK;
}

// the single entries: validation shared by the query and the call; *rq <- the residual-only request
static int single_plan(const char* who, int family, const pinn_desc* desc, const pinn_residual_spec* spec, int64_t N, Net* n,
                       LossReq* rq, int* engine) {
  int rc = make_net(desc, n); if (rc) return rc;
  rc = build_request(*n, spec, N, N, 0, 0, nullptr, rq); if (rc) return rc;
  return extra_rules(who, family, family == TILE_WEIGHTED, true, desc, *n, spec, engine);
}
static int32_t single_query(const char* who, int family, const pinn_desc* desc, const pinn_residual_spec* spec, int64_t N, int64_t* bytes) {
  Net n; LossReq rq; int e;
  int rc = single_plan(who, family, desc, spec, N, &n, &rq, &e); if (rc) return rc;
  if (!bytes || N < 0) { set_error("bad arguments"); return PINN_ERR_INVALID; }
  const int64_t b = e == PINN_ENGINE_FUSED ? fused_tile_workspace_bytes(family, n, N) : generic_workspace_bytes(n, N);
  if (b < 0) { set_error("network not supported"); return PINN_ERR_UNSUPPORTED; }
  *bytes = b;
  return PINN_OK;
}
static int32_t single_run(int family, int e, const Net& n, const LossReq& rq, const float* params, const float* X, int64_t N,
                          void* ws, int64_t ws_bytes, hipStream_t s) {
  if (N == 0) { (void)hipMemsetAsync(rq.sums, 0, rq.n_terms * sizeof(float), s); return PINN_OK; }
  return e == PINN_ENGINE_FUSED ? fused_tile_loss(family, n, rq, params, X, N, ws, ws_bytes, s)
                                : generic_loss(n, rq, params, X, N, ws, ws_bytes, s);
}

int32_t pinn_query_residual_coef_workspace(const pinn_desc* desc, const pinn_residual_spec* spec, int64_t N, int64_t* bytes) {
  return single_query("pinn_residual_coef_loss_grad", TILE_COEF, desc, spec, N, bytes);
}

int32_t pinn_residual_coef_loss_grad(const pinn_desc* desc, const pinn_residual_spec* spec, const float* coef,
                                     const float* term_scale, const float* params, const float* X, int64_t N,
                                     float* term_sums, float* grad_flat, float* coef_grad, void* ws, int64_t ws_bytes,
                                     void* stream) {
  Net n; LossReq rq; int e;
  int rc = single_plan("pinn_residual_coef_loss_grad", TILE_COEF, desc, spec, N, &n, &rq, &e); if (rc) return rc;
  if (!coef || !params || (!X && N > 0) || N < 0 || !term_sums || (grad_flat && !term_scale)) {
    set_error("NULL pointer argument"); return PINN_ERR_INVALID;
  }
  if (coef_grad && !grad_flat) { set_error("coef_grad without grad_flat: the coefficient gradient comes out of the gradient pass"); return PINN_ERR_INVALID; }
  rq.scale = term_scale; rq.sums = term_sums; rq.grad = grad_flat;
  rq.coef = coef; rq.coef_grad = coef_grad; rq.n_coef = 1;
  return single_run(TILE_COEF, e, n, rq, params, X, N, ws, ws_bytes, (hipStream_t)stream);
}

// ---- per-point weights on the residual's squares -------------------------------------------------------------------------
int32_t pinn_query_residual_weighted_workspace(const pinn_desc* desc, const pinn_residual_spec* spec, int64_t N, int64_t* bytes) {
  return single_query("pinn_residual_weighted_loss_grad", TILE_WEIGHTED, desc, spec, N, bytes);
}

int32_t pinn_residual_weighted_loss_grad(const pinn_desc* desc, const pinn_residual_spec* spec, const float* term_scale,
                                         const float* point_w, int32_t w_rows, const float* params, const float* X,
                                         int64_t N, float* term_sums, float* fields, float* grad_flat, void* ws,
                                         int64_t ws_bytes, void* stream) {
  Net n; LossReq rq; int e;
  int rc = single_plan("pinn_residual_weighted_loss_grad", TILE_WEIGHTED, desc, spec, N, &n, &rq, &e); if (rc) return rc;
  const int n_w = residual_n_weighted(spec->residual_id);
  if (!point_w) { set_error("pinn_residual_weighted_loss_grad: point_w is NULL"); return PINN_ERR_INVALID; }
  if (w_rows != 1 && w_rows != n_w) {
    set_error("pinn_residual_weighted_loss_grad: w_rows = %d, residual %d takes 1 row or %d (one per weighted term)", w_rows,
              spec->residual_id, n_w);
    return PINN_ERR_INVALID;
  }
  if (!params || (!X && N > 0) || N < 0 || !term_sums || (grad_flat && !term_scale)) {
    set_error("NULL pointer argument"); return PINN_ERR_INVALID;
  }
  rq.scale = term_scale; rq.sums = term_sums; rq.grad = grad_flat;
  rq.point_w = point_w; rq.w_stride = w_rows == 1 ? 0 : N; rq.n_weighted = n_w; rq.fields_out = fields;
  return single_run(TILE_WEIGHTED, e, n, rq, params, X, N, ws, ws_bytes, (hipStream_t)stream);
}

// ---- device-enqueued Adam runs with coefficients or point weights (pinn_hip.h; kernels: pinn_fused.hip) -------------------
// validation shared by the query and the call, in the order of the header's table (no HIP call before it has passed);
// *res <- the residual pass's request with the group's arrays (coef set: the request carries coefficients, else weights)
static int adam_ext_plan(const char* who, const pinn_desc* desc, const pinn_residual_spec* spec, const pinn_adam_extras* ex,
                         int64_t N_res, int64_t N_fid, Net* n, LossReq* res) {
  int rc = make_net(desc, n); if (rc) return rc;
  rc = build_request(*n, spec, N_res, N_res, 0, 0, nullptr, res); if (rc) return rc;
  if (!ex) { set_error("%s: extras is NULL (use pinn_adam_loop for the plain request)", who); return PINN_ERR_INVALID; }
  if (ex->coef && ex->point_w) {
    set_error("%s: coefficients and point weights together: no kernel carries both", who); return PINN_ERR_UNSUPPORTED;
  }
  if (!ex->coef && !ex->point_w) {
    set_error("%s: neither coef nor point_w is given (use pinn_adam_loop for the plain request)", who); return PINN_ERR_INVALID;
  }
  int e;
  rc = extra_rules(who, ex->coef ? TILE_COEF : TILE_WEIGHTED, false, false, desc, *n, spec, &e); if (rc) return rc;
  if (ex->coef) { res->coef = ex->coef; res->coef_grad = ex->coef_grad; res->n_coef = 1; }
  else {
    const int n_w = residual_n_weighted(spec->residual_id);
    if (ex->w_rows != 1 && ex->w_rows != n_w) {
      set_error("%s: w_rows = %d, residual %d takes 1 row or %d (one per weighted term)", who, ex->w_rows, spec->residual_id, n_w);
      return PINN_ERR_INVALID;
    }
    if (ex->lam && ex->sa_mask != 0 && ex->sa_mask != 1) { set_error("%s: sa_mask = %d (0: w = lam^2, 1: w = lam)", who, ex->sa_mask); return PINN_ERR_INVALID; }
    res->point_w = ex->point_w; res->w_stride = ex->w_rows == 1 ? 0 : N_res; res->n_weighted = n_w; res->fields_out = ex->fields;
  }
  if (N_res < 1 || N_fid < 0) { set_error("%s: N_res = %lld must be >= 1, N_fid = %lld >= 0", who, (long long)N_res, (long long)N_fid); return PINN_ERR_INVALID; }
  return PINN_OK;
}

int32_t pinn_query_adam_ext_workspace(const pinn_desc* desc, const pinn_residual_spec* spec, const pinn_adam_extras* extras,
                                      int64_t N_res, int64_t N_fid, int64_t* bytes) {
  Net n; LossReq res;
  int rc = adam_ext_plan("pinn_query_adam_ext_workspace", desc, spec, extras, N_res, N_fid, &n, &res); if (rc) return rc;
  if (!bytes) { set_error("bytes is NULL"); return PINN_ERR_INVALID; }
  *bytes = fused_adam_ext_workspace_bytes(n, N_res, N_fid);
  return PINN_OK;
}

int32_t pinn_adam_loop_ext(const pinn_desc* desc, const pinn_residual_spec* spec, const float* term_scale,
                           const float* Xf, const float* T, int64_t N_fid, int32_t n_cols, const int32_t* out_col,
                           const float* col_scale, float* params, const float* X, int64_t N_res,
                           float* term_sums, float* col_sums, float* grad_flat, const pinn_adam_state* adam,
                           const pinn_adam_extras* extras, int32_t n_iters, const double* lr, const double* lr_coef,
                           const double* lr_w, void* ws, int64_t ws_bytes, void* stream) {
  const char* who = "pinn_adam_loop_ext";
  Net n; AdamExtReq q; memset(&q, 0, sizeof(q));
  LossReq& r = q.res;
  int rc = adam_ext_plan(who, desc, spec, extras, N_res, N_fid, &n, &r); if (rc) return rc;
  const bool coef = r.coef != nullptr;
  if (!adam || n_iters < 0) { set_error("%s: bad arguments", who); return PINN_ERR_INVALID; }
  if (n_iters == 0) return PINN_OK;
  if (!params || !X || !term_sums || !term_scale || !grad_flat || !adam->m || !adam->v || adam->step < 1 || !lr) {
    set_error("%s: bad arguments", who); return PINN_ERR_INVALID;
  }
  if (n_cols < 0 || n_cols > PINN_MAX_ROLES) { set_error("n_cols=%d outside 0..%d", n_cols, PINN_MAX_ROLES); return PINN_ERR_INVALID; }
  if (N_fid > 0 && (n_cols < 1 || !Xf || !T || !out_col || !col_scale || !col_sums)) {
    set_error("%s: fidelity points need n_cols >= 1, Xf, T, out_col, col_scale and col_sums", who); return PINN_ERR_INVALID;
  }
  rc = adam_req(adam, params, &q.adam); if (rc) return rc;
  if (coef && extras->coef_grad && (!extras->coef_m || !extras->coef_v || !lr_coef)) {
    set_error("%s: trainable coefficients need coef_m, coef_v and lr_coef", who); return PINN_ERR_INVALID;
  }
  if (!coef && extras->lam && (!extras->lam_m || !extras->lam_v || !extras->fields || !lr_w)) {
    set_error("%s: self-adaptive weights need lam_m, lam_v, fields and lr_w", who); return PINN_ERR_INVALID;
  }
  r.scale = term_scale; r.sums = term_sums; r.grad = grad_flat;
  if (N_fid > 0) {
    LossReq& m = q.fid;
    m.kind = 1; m.n_split = -1; m.T = T; m.n_cols = n_cols; m.mse_scale = col_scale; m.mse_sums = col_sums; m.grad = grad_flat;
    rc = set_out_cols(n, n_cols, out_col, &m); if (rc) return rc;
  }
  q.Xf = Xf; q.N_fid = N_fid;
  q.beta1 = adam->beta1; q.beta2 = adam->beta2; q.eps = adam->eps; q.step = adam->step;
  q.row_cols = n_cols; q.col_sums = col_sums;
  if (coef) {
    q.coef = extras->coef; q.coef_m = extras->coef_m; q.coef_v = extras->coef_v; q.coef_grad = extras->coef_grad;
    q.coef_mask = extras->coef_mask; q.coef_log = extras->coef_log; q.n_coef = 1;
  } else {
    q.point_w = extras->point_w; q.w_rows = extras->w_rows; q.lam = extras->lam; q.lam_m = extras->lam_m; q.lam_v = extras->lam_v;
    q.sa_mask = extras->sa_mask;
  }
  q.n_iters = n_iters; q.lr = lr; q.lr_coef = lr_coef; q.lr_w = lr_w;
  return fused_adam_ext(n, q, X, N_res, ws, ws_bytes, (hipStream_t)stream);
}

// ---- gradient-statistics loss balancing (pinn_hip.h; the rule and the reductions: balance.h) -------------------------------
// the rule's arguments, checked once for the host entry, the flat-gradient entry and the balanced loop
static int balance_args(const char* who, int mode, bool allow_none, int G, int ref, double alpha, int64_t P) {
  if (mode != PINN_BALANCE_MAX_MEAN && mode != PINN_BALANCE_NORM && !(allow_none && mode == PINN_BALANCE_NONE)) {
    set_error("%s: unknown mode %d (%s1 = max/mean, 2 = gradient norm)", who, mode, allow_none ? "0 = combine only, " : ""); return PINN_ERR_INVALID;
  }
  if (G < 1 || G > PINN_BALANCE_MAX_GROUPS) { set_error("%s: G = %d outside 1..%d", who, G, PINN_BALANCE_MAX_GROUPS); return PINN_ERR_INVALID; }
  if (ref < 0 || ref >= G) { set_error("%s: ref = %d outside 0..%d", who, ref, G - 1); return PINN_ERR_INVALID; }
  if (!(alpha > 0.0 && alpha <= 1.0)) { set_error("%s: alpha = %g outside (0, 1]", who, alpha); return PINN_ERR_INVALID; }
  if (P < 1) { set_error("%s: P = %lld must be >= 1", who, (long long)P); return PINN_ERR_INVALID; }
  return PINN_OK;
}

int32_t pinn_balance_weights_host(int32_t mode, int32_t G, int32_t ref, double alpha, int64_t P, const double* stats,
                                  const float* lam_in, float* lam_out) {
  const char* who = "pinn_balance_weights_host";
  int rc = balance_args(who, mode, true, G, ref, alpha, P); if (rc) return rc;
  if (!lam_in || !lam_out || (!stats && mode != PINN_BALANCE_NONE)) { set_error("%s: NULL pointer argument", who); return PINN_ERR_INVALID; }
  float in[PINN_BALANCE_MAX_GROUPS];
  for (int j = 0; j < G; ++j) in[j] = lam_in[j];   // (lam_out may be lam_in)
  balance_weights(mode, G, ref, alpha, P, stats, in, lam_out);
  return PINN_OK;
}

int32_t pinn_query_balance_workspace(int64_t P, int32_t G, int64_t* bytes) {
  const char* who = "pinn_query_balance_workspace";
  int rc = balance_args(who, PINN_BALANCE_NONE, true, G, 0, 1.0, P); if (rc) return rc;
  if (!bytes) { set_error("%s: bytes is NULL", who); return PINN_ERR_INVALID; }
  *bytes = balance_workspace_bytes(P, G);
  return PINN_OK;
}

int32_t pinn_balance_update(int32_t mode, int32_t G, int32_t ref, double alpha, const float* grads, int64_t P, int64_t ld,
                            float* lam, double* stats, float* grad_out, void* ws, int64_t ws_bytes, void* stream) {
  const char* who = "pinn_balance_update";
  int rc = balance_args(who, mode, true, G, ref, alpha, P); if (rc) return rc;
  if (ld < P) { set_error("%s: ld = %lld is below P = %lld", who, (long long)ld, (long long)P); return PINN_ERR_INVALID; }
  if (!grads || !lam) { set_error("%s: grads or lam is NULL", who); return PINN_ERR_INVALID; }
  if (mode != PINN_BALANCE_NONE) { rc = check_workspace(ws, ws_bytes, balance_workspace_bytes(P, G)); if (rc) return rc; }
  return balance_update(mode, G, ref, alpha, grads, P, ld, lam, stats, grad_out, ws, (hipStream_t)stream);
}

// validation shared by the balanced loop's query and call, next to adam_ext_plan and in the order of the header's table (no
// HIP call before it has passed); bal may be null in the query only; *res <- the plain residual pass's request
static int adam_bal_plan(const char* who, bool query, const pinn_desc* desc, const pinn_residual_spec* spec, const pinn_balance* bal,
                         int64_t N_res, int64_t N_fid, Net* n, LossReq* res) {
  int rc = make_net(desc, n); if (rc) return rc;
  rc = build_request(*n, spec, N_res, N_res, 0, 0, nullptr, res); if (rc) return rc;
  if (is_corrected(spec->residual_id, spec->flags)) {
    set_error("%s: %s has no natural-order pass in the balanced loop", who, pe_closure_name((spec->flags & 2) != 0));
    return PINN_ERR_UNSUPPORTED;
  }
  rc = check_k(who, *n, spec, ""); if (rc) return rc;
  if (n->prec != PINN_PREC_F32) { set_error("%s is implemented in fp32 only (precision bf16 refused)", who); return PINN_ERR_UNSUPPORTED; }
  const int asked = asked_engine(desc);
  if (asked == PINN_ENGINE_GENERIC || asked == PINN_ENGINE_WIDE) {
    set_error("%s runs on the fused engine only (engine AUTO, FUSED, FUSED_TILE or FUSED_COOP), not on engine %d: use the loss "
              "calls, pinn_balance_update and pinn_adam_step", who, desc->engine);
    return PINN_ERR_UNSUPPORTED;
  }
  if (const char* why = fused_adam_bal_refusal(*n)) {
    set_error("%s: %s (width %d, d_in %d, d_out %d, k %d, activation %d, dropout_p %g); use the loss calls, pinn_balance_update "
              "and pinn_adam_step", who, why, n->W, n->d_in, n->d_out, n->k, n->act, (double)n->drop_p);
    return PINN_ERR_UNSUPPORTED;
  }
  if (N_res < 1 || N_fid < 1) { set_error("%s: N_res = %lld and N_fid = %lld must be >= 1", who, (long long)N_res, (long long)N_fid); return PINN_ERR_INVALID; }
  if (query && !bal) return PINN_OK;
  if (!bal || !bal->lam) { set_error("%s: balance or balance->lam is NULL", who); return PINN_ERR_INVALID; }
  if (bal->every < 1) { set_error("%s: every = %d must be >= 1", who, bal->every); return PINN_ERR_INVALID; }
  return balance_args(who, bal->mode, false, 2, bal->ref, bal->alpha, 1);
}

int32_t pinn_query_adam_balanced_workspace(const pinn_desc* desc, const pinn_residual_spec* spec, int64_t N_res, int64_t N_fid,
                                           int64_t* bytes) {
  Net n; LossReq res;
  int rc = adam_bal_plan("pinn_query_adam_balanced_workspace", true, desc, spec, nullptr, N_res, N_fid, &n, &res); if (rc) return rc;
  if (!bytes) { set_error("bytes is NULL"); return PINN_ERR_INVALID; }
  *bytes = fused_adam_bal_workspace_bytes(n, N_res, N_fid);
  return PINN_OK;
}

int32_t pinn_adam_loop_balanced(const pinn_desc* desc, const pinn_residual_spec* spec, const float* term_scale,
                                const float* Xf, const float* T, int64_t N_fid, int32_t n_cols, const int32_t* out_col,
                                const float* col_scale, float* params, const float* X, int64_t N_res,
                                float* term_sums, float* col_sums, float* grad_flat, const pinn_adam_state* adam,
                                const pinn_balance* balance, int32_t n_iters, const double* lr,
                                void* ws, int64_t ws_bytes, void* stream) {
  const char* who = "pinn_adam_loop_balanced";
  Net n; AdamBalReq q; memset(&q, 0, sizeof(q));
  LossReq& r = q.res;
  int rc = adam_bal_plan(who, false, desc, spec, balance, N_res, N_fid, &n, &r); if (rc) return rc;
  if (!adam || n_iters < 0) { set_error("%s: bad arguments", who); return PINN_ERR_INVALID; }
  if (n_iters == 0) return PINN_OK;
  if (!params || !X || !term_sums || !term_scale || !grad_flat || !adam->m || !adam->v || adam->step < 1 || !lr) {
    set_error("%s: bad arguments", who); return PINN_ERR_INVALID;
  }
  if (n_cols < 1 || n_cols > PINN_MAX_ROLES || !Xf || !T || !out_col || !col_scale || !col_sums) {
    set_error("%s: the fidelity group needs n_cols in 1..%d, Xf, T, out_col, col_scale and col_sums", who, PINN_MAX_ROLES); return PINN_ERR_INVALID;
  }
  rc = adam_req(adam, params, &q.adam); if (rc) return rc;
  r.scale = term_scale; r.sums = term_sums; r.grad = grad_flat;
  LossReq& m = q.fid;
  m.kind = 1; m.n_split = -1; m.T = T; m.n_cols = n_cols; m.mse_scale = col_scale; m.mse_sums = col_sums; m.grad = grad_flat;
  rc = set_out_cols(n, n_cols, out_col, &m); if (rc) return rc;
  q.Xf = Xf; q.N_fid = N_fid;
  q.beta1 = adam->beta1; q.beta2 = adam->beta2; q.eps = adam->eps; q.step = adam->step;
  q.row_cols = n_cols; q.col_sums = col_sums;
  q.mode = balance->mode; q.every = balance->every; q.ref = balance->ref; q.alpha = balance->alpha;
  q.lam = balance->lam; q.lam_log = balance->lam_log; q.stats_log = balance->stats_log; q.group_grads = balance->group_grads;
  q.n_iters = n_iters; q.lr = lr;
  return fused_adam_bal(n, q, X, N_res, ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"
