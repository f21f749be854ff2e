// extern "C" boundary of libfastscnn_hip.so (declared in include/fastscnn.h).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>

#include "../../include/fastscnn.h"
#include "net.hpp"

namespace fscnn {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}
const char* last_error() { return g_err; }

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return E_HIP;
  }
  return OK;
}

// ---- launch profiler --------------------------------------------------------------------
unsigned long long* g_stamps = nullptr;
int g_prof_kind = PK_NONE;
thread_local const char* g_prof_tag = "";
namespace {
struct ProfState {
  std::vector<hipEvent_t> ev;  // pairs
  std::vector<int> kind;       // per recorded launch
  std::vector<std::string> tag;
  std::vector<double> lbytes, lflops;
  size_t used = 0;
  double bytes = 0, flops = 0;
  long long launches = 0;
  bool overflow = false;
  bool armed = false, taken = false;  // the open scope's events (prof_start / prof_take_ext)
  hipStream_t arm_st = nullptr;
} g_prof;
}  // namespace

bool g_host_prof = env_on("FSCNN_HOST_PROF", false);
namespace {
struct HostProf {
  double us[4] = {0, 0, 0, 0};
  long long n[4] = {0, 0, 0, 0};
  ~HostProf() {
    if (!g_host_prof) return;
    static const char* names[4] = {"kernel launches", "side-stream forks", "side-stream joins",
                                   "C entry points (total)"};
    for (int i = 0; i < 4; ++i)
      fprintf(stderr, "FSCNN_HOST_PROF %-24s %10lld calls %12.1f us  (%.2f us each)\n", names[i],
              n[i], us[i], n[i] ? us[i] / n[i] : 0.0);
  }
} g_hostp;
}  // namespace
double host_now_us() {
  return std::chrono::duration<double, std::micro>(
             std::chrono::steady_clock::now().time_since_epoch()).count();
}
void host_prof_add(int what, double us) {
  g_hostp.us[what] += us;
  g_hostp.n[what]++;
}

// A scope arms its event pair for the first prof_launch inside it (kernel-bound events); a scope
// whose launch does not take them (none issued) falls back to marker events around the scope.
void prof_start(hipStream_t st) {
  if (g_prof.used + 2 > g_prof.ev.size()) { g_prof.overflow = true; return; }
  g_prof.armed = true;
  g_prof.taken = false;
  g_prof.arm_st = st;
}
bool prof_take_ext(hipEvent_t& e0, hipEvent_t& e1) {
  if (!g_prof.armed || g_prof.taken) return false;
  e0 = g_prof.ev[g_prof.used];
  e1 = g_prof.ev[g_prof.used + 1];
  g_prof.taken = true;
  return true;
}
void prof_stop(hipStream_t st, int kind, double bytes, double flops) {
  if (g_prof.used + 2 > g_prof.ev.size()) return;
  const bool taken = g_prof.armed && g_prof.taken;
  g_prof.armed = false;
  if (!taken) {  // no kernel launched in the scope: a zero-length marker pair
    (void)hipEventRecord(g_prof.ev[g_prof.used], st);
    (void)hipEventRecord(g_prof.ev[g_prof.used + 1], st);
  }
  g_prof.used += 2;
  g_prof.kind.push_back(kind);
  g_prof.tag.emplace_back(g_prof_tag ? g_prof_tag : "");
  g_prof.lbytes.push_back(bytes);
  g_prof.lflops.push_back(flops);
  g_prof.bytes += bytes;
  g_prof.flops += flops;
  g_prof.launches++;
}

}  // namespace fscnn

using namespace fscnn;

extern "C" int fscnn_prof_begin(int kind, int max_launches) {
  if ((kind <= PK_NONE || kind >= PK_COUNT) && kind != PK_ALL) {
    set_error("fscnn_prof_begin: bad kind %d", kind);
    return E_INVALID;
  }
  if (max_launches <= 0) {
    set_error("fscnn_prof_begin: bad kind %d", kind);
    return E_INVALID;
  }
  size_t need = (size_t)max_launches * 2;
  while (g_prof.ev.size() < need) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) { set_error("hipEventCreate failed"); return E_HIP; }
    g_prof.ev.push_back(e);
  }
  g_prof.used = 0; g_prof.bytes = 0; g_prof.flops = 0; g_prof.launches = 0;
  g_prof.kind.clear(); g_prof.tag.clear(); g_prof.lbytes.clear(); g_prof.lflops.clear();
  g_prof.overflow = false;
  g_prof_kind = kind;
  return OK;
}

// Synchronises on the recorded events; returns summed kernel time (ms), launches and the
// algorithmic bytes / flops of those launches.
extern "C" int fscnn_prof_end(double* total_ms, long long* launches, double* bytes, double* flops) {
  g_prof_kind = PK_NONE;
  double tot = 0;
  for (size_t i = 0; i + 1 < g_prof.used; i += 2) {
    float ms = 0;
    if (hipEventSynchronize(g_prof.ev[i + 1]) != hipSuccess ||
        hipEventElapsedTime(&ms, g_prof.ev[i], g_prof.ev[i + 1]) != hipSuccess) {
      set_error("fscnn_prof_end: event query failed");
      return E_HIP;
    }
    tot += ms;
  }
  if (total_ms) *total_ms = tot;
  if (launches) *launches = g_prof.launches;
  if (bytes) *bytes = g_prof.bytes;
  if (flops) *flops = g_prof.flops;
  if (g_prof.overflow) { set_error("fscnn_prof_end: event pool overflow"); return E_INVALID; }
  return OK;
}

// One recorded launch of the last fscnn_prof_begin / _end window (after _end): its kind, kernel
// time, algorithmic bytes / flops and the executor's layer label.
extern "C" int fscnn_prof_launch(long long i, int* kind, float* ms, double* bytes, double* flops,
                                 const char** tag) {
  if (i < 0 || (size_t)i >= g_prof.kind.size()) {
    set_error("fscnn_prof_launch: index %lld out of range (%zu recorded)", i, g_prof.kind.size());
    return E_INVALID;
  }
  float t = 0;
  if (hipEventElapsedTime(&t, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]) != hipSuccess) {
    set_error("fscnn_prof_launch: event query failed");
    return E_HIP;
  }
  if (kind) *kind = g_prof.kind[i];
  if (ms) *ms = t;
  if (bytes) *bytes = g_prof.lbytes[i];
  if (flops) *flops = g_prof.lflops[i];
  if (tag) *tag = g_prof.tag[i].c_str();  // valid until the next fscnn_prof_begin
  return OK;
}

// Phase stamps of the next launches of the instrumented kernels (pointwise GEMMs, depthwise
// forward / stride-1 dgrad): launch i writes buf + i * STAMP_STRIDE (max_launches regions; null:
// off).  Debug / tools only (process-global, single thread).
namespace fscnn {
static int g_stamp_max = 0, g_stamp_used = 0;
static std::vector<std::string> g_stamp_tags;
unsigned long long* stamp_region() {
  if (!g_stamps || g_stamp_used >= g_stamp_max) return nullptr;
  g_stamp_tags.emplace_back(g_prof_tag ? g_prof_tag : "");
  return g_stamps + (size_t)(g_stamp_used++) * STAMP_STRIDE;
}
}  // namespace fscnn
extern "C" int fscnn_debug_stamps(void* buf, int max_launches) {
  g_stamps = reinterpret_cast<unsigned long long*>(buf);
  g_stamp_max = buf ? max_launches : 0;
  g_stamp_used = 0;
  g_stamp_tags.clear();
  return OK;
}
extern "C" int fscnn_debug_stamp_count(void) { return g_stamp_used; }
extern "C" const char* fscnn_debug_stamp_tag(int i) {
  return (i >= 0 && i < (int)g_stamp_tags.size()) ? g_stamp_tags[i].c_str() : "";
}

extern "C" const char* fscnn_prof_kind_name(int kind) {
  static const char* names[PK_COUNT] = {"none", "conv0_fwd", "dw_fwd", "dw_dgrad", "dw_wgrad",
                                        "gemm_nt", "gemm_tn", "bn_apply", "bn_bwd", "upsample",
                                        "upsample_bwd", "cross_entropy", "conv0_wgrad",
                                        "bn_bwd_reduce", "bn_finalize", "ppm_branches",
                                        "ir_block", "ltd_stem", "dsconv"};
  return (kind >= 0 && kind < PK_COUNT) ? names[kind] : "?";
}

struct fscnn_net {
  Net net;
};
struct fscnn_plan {
  Plan plan;
};

#define GUARD(expr)                                   \
  try {                                               \
    return (expr);                                    \
  } catch (const std::exception& e) {                 \
    set_error("exception: %s", e.what());             \
    return E_INVALID;                                 \
  }

static hipStream_t S(void* s) { return (hipStream_t)s; }

// What every whole-network entry passes to net_forward / net_backward alike; an entry adds its own
// outputs and head fields.  out_dtype is the plan's (the two entries that write logits set the
// caller's); the inference entries pass seed 0, dropout_p 0 and momentum 0.1f.
static RunArgs forward_args(const Plan& pl, const void* x, int x_dtype, const float* params,
                            float* running, long long* nbt, void* ws, unsigned long long seed,
                            float dropout_p, float momentum, void* stream) {
  RunArgs r{};
  r.x = x; r.x_dtype = x_dtype; r.out_dtype = pl.dtype;
  r.P = params; r.R = running; r.NBT = nbt; r.ws = ws;
  r.seed = seed; r.dropout_p = dropout_p; r.momentum = momentum; r.st = S(stream);
  return r;
}

static RunArgs backward_args(const void* x, int x_dtype, const float* params, float* grads,
                             void* ws, void* bws, unsigned long long seed, float dropout_p,
                             void* stream) {
  RunArgs r{};
  r.x = x; r.x_dtype = x_dtype; r.P = params; r.G = grads; r.ws = ws; r.bws = bws;
  r.seed = seed; r.dropout_p = dropout_p; r.st = S(stream);
  return r;
}

extern "C" {

const char* fscnn_version(void) { return "fastscnn-hip 0.1 (gfx950)"; }
const char* fscnn_last_error(void) { return last_error(); }

int fscnn_net_create(int num_classes, int aux, fscnn_net** out) {
  if (!out) { set_error("fscnn_net_create: null out"); return E_INVALID; }
  fscnn_net* n = new (std::nothrow) fscnn_net();
  if (!n) { set_error("fscnn_net_create: out of host memory"); return E_INVALID; }
  int rc = net_build(num_classes, aux, n->net);
  if (rc) { delete n; return rc; }
  *out = n;
  return OK;
}
void fscnn_net_destroy(fscnn_net* net) { delete net; }

int fscnn_net_param_count(const fscnn_net* net, int* count, long long* total) {
  if (!net) { set_error("null net"); return E_INVALID; }
  if (count) *count = (int)net->net.params.size();
  if (total) *total = net->net.p_total;
  return OK;
}
int fscnn_net_param_info(const fscnn_net* net, int i, const char** name, long long* offset,
                         long long* numel) {
  if (!net || i < 0 || i >= (int)net->net.params.size()) { set_error("bad param index %d", i); return E_INVALID; }
  const TSpec& t = net->net.params[i];
  if (name) *name = t.name.c_str();
  if (offset) *offset = t.off;
  if (numel) *numel = t.numel;
  return OK;
}
int fscnn_net_buffer_count(const fscnn_net* net, int* count, long long* total, int* num_bn) {
  if (!net) { set_error("null net"); return E_INVALID; }
  if (count) *count = (int)net->net.buffers.size();
  if (total) *total = net->net.r_total;
  if (num_bn) *num_bn = net->net.n_bn;
  return OK;
}
int fscnn_net_buffer_info(const fscnn_net* net, int i, const char** name, long long* offset,
                          long long* numel) {
  if (!net || i < 0 || i >= (int)net->net.buffers.size()) { set_error("bad buffer index %d", i); return E_INVALID; }
  const TSpec& t = net->net.buffers[i];
  if (name) *name = t.name.c_str();
  if (offset) *offset = t.off;
  if (numel) *numel = t.numel;
  return OK;
}
int fscnn_net_stage_range(const fscnn_net* net, int stage, long long* begin, long long* end) {
  if (!net || stage < 0 || stage > 3) { set_error("bad stage %d", stage); return E_INVALID; }
  const Net& n = net->net;
  *begin = n.stage_p_begin[stage];
  *end = stage == 0 ? n.p_total : n.stage_p_begin[stage - 1];
  return OK;
}

int fscnn_plan_create(const fscnn_net* net, int N, int H, int W, int dtype, int train,
                      fscnn_plan** out) {
  if (!net || !out) { set_error("fscnn_plan_create: null argument"); return E_INVALID; }
  fscnn_plan* p = new (std::nothrow) fscnn_plan();
  if (!p) { set_error("out of host memory"); return E_INVALID; }
  int rc = plan_build(net->net, N, H, W, dtype, train, p->plan);
  if (rc) { delete p; return rc; }
  p->plan.graphs = make_graph_cache();
  p->plan.side = make_side_stream();
  *out = p;
  return OK;
}
void fscnn_plan_destroy(fscnn_plan* plan) { delete plan; }
int fscnn_plan_workspace(const fscnn_plan* plan, long long* fwd, long long* bwd) {
  if (!plan) { set_error("null plan"); return E_INVALID; }
  if (fwd) *fwd = (long long)plan->plan.ws_bytes;
  if (bwd) *bwd = (long long)plan->plan.bws_bytes;
  return OK;
}
int fscnn_plan_shapes(const fscnn_plan* plan, int* d) {
  if (!plan || !d) { set_error("null plan"); return E_INVALID; }
  const Plan& p = plan->plan;
  int v[10] = {p.H1, p.W1, p.H2, p.W2, p.H3, p.W3, p.H4, p.W4, p.H5, p.W5};
  memcpy(d, v, sizeof v);
  return OK;
}

int fscnn_forward(const fscnn_plan* plan, const void* x, int x_dtype, void* out, int out_dtype,
                  const float* params, float* running, long long* nbt, void* ws,
                  unsigned long long seed, float dropout_p, float momentum, void* stream) {
  if (!plan || !x || !out || !params || !running || !ws) {
    set_error("fscnn_forward: null argument");
    return E_INVALID;
  }
  RunArgs r = forward_args(plan->plan, x, x_dtype, params, running, nbt, ws, seed, dropout_p,
                           momentum, stream);
  r.out = out; r.out_dtype = out_dtype;
  GUARD(net_forward(plan->plan, r));
}

int fscnn_backward(const fscnn_plan* plan, const void* dout, const void* x, int x_dtype,
                   const float* params, float* grads, void* ws, void* bws,
                   unsigned long long seed, float dropout_p, int stage_from, int stage_to,
                   void* stream) {
  if (!plan || !dout || !x || !params || !grads || !ws || !bws) {
    set_error("fscnn_backward: null argument");
    return E_INVALID;
  }
  RunArgs r = backward_args(x, x_dtype, params, grads, ws, bws, seed, dropout_p, stream);
  r.dout = dout;
  GUARD(net_backward(plan->plan, r, stage_from, stage_to));
}

int fscnn_forward_aux(const fscnn_plan* plan, const void* x, int x_dtype, void* out, void* aux_out,
                      int out_dtype, const float* params, float* running, long long* nbt,
                      void* ws, unsigned long long seed, float dropout_p, float momentum,
                      void* stream) {
  if (!plan || !x || !out || !aux_out || !params || !running || !ws) {
    set_error("fscnn_forward_aux: null argument");
    return E_INVALID;
  }
  RunArgs r = forward_args(plan->plan, x, x_dtype, params, running, nbt, ws, seed, dropout_p,
                           momentum, stream);
  r.out = out; r.aux_out = aux_out; r.out_dtype = out_dtype;
  GUARD(net_forward(plan->plan, r));
}

int fscnn_backward_aux(const fscnn_plan* plan, const void* dout, const void* daux, const void* x,
                       int x_dtype, const float* params, float* grads, void* ws, void* bws,
                       unsigned long long seed, float dropout_p, int stage_from, int stage_to,
                       void* stream) {
  if (!plan || !dout || !daux || !x || !params || !grads || !ws || !bws) {
    set_error("fscnn_backward_aux: null argument");
    return E_INVALID;
  }
  RunArgs r = backward_args(x, x_dtype, params, grads, ws, bws, seed, dropout_p, stream);
  r.dout = dout; r.daux = daux;
  GUARD(net_backward(plan->plan, r, stage_from, stage_to));
}

int fscnn_predict(const fscnn_plan* plan, const void* x, int x_dtype, void* labels,
                  int label_dtype, const float* params, float* running, long long* nbt, void* ws,
                  void* stream) {
  if (!plan || !x || !labels || !params || !running || !ws) {
    set_error("fscnn_predict: null argument");
    return E_INVALID;
  }
  if (plan->plan.train) {
    set_error("fscnn_predict: needs an inference plan (train=0)");
    return E_INVALID;
  }
  if (label_dtype != 0 && label_dtype != 1) {
    set_error("fscnn_predict: label_dtype %d (0 int64, 1 uint8)", label_dtype);
    return E_INVALID;
  }
  RunArgs r = forward_args(plan->plan, x, x_dtype, params, running, nbt, ws, 0, 0.f, 0.1f, stream);
  r.labels = labels; r.label_u8 = label_dtype;
  GUARD(net_forward(plan->plan, r));
}

long long fscnn_validate_ws_bytes(const fscnn_plan* plan) {
  if (!plan || plan->plan.train) {
    set_error("fscnn_validate_ws_bytes: the validation head needs an inference plan (train=0)");
    return E_INVALID;
  }
  const Plan& pl = plan->plan;
  return (long long)eval_head_parts(pl.N, pl.H, pl.W) * 4 * (long long)sizeof(float);
}

int fscnn_validate(const fscnn_plan* plan, const void* x, int x_dtype, const long long* target,
                   int head, long long ignore_index, float smooth, float dice_weight,
                   float focal_weight, float alpha, float gamma, float aux_weight, float* loss,
                   long long* counts, const float* params, float* running, long long* nbt,
                   void* ws, void* head_ws, void* stream) {
  if (!plan || !x || !target || !loss || !params || !running || !ws || !head_ws) {
    set_error("fscnn_validate: null argument");
    return E_INVALID;
  }
  const Plan& pl = plan->plan;
  if (pl.train) {
    set_error("fscnn_validate: needs an inference plan (train=0)");
    return E_INVALID;
  }
  if (head != HEAD_CE && head != HEAD_DICE) {
    set_error("fscnn_validate: head %d (0 cross entropy, 1 dice)", head);
    return E_INVALID;
  }
  if (aux_weight != 0.f && !pl.net->aux) {
    set_error("fscnn_validate: aux_weight without an aux net");
    return E_INVALID;
  }
  if (!eval_head_ok(pl.N, pl.net->num_classes, pl.H3, pl.W3, pl.H, pl.W, head == HEAD_DICE)) {
    set_error("fscnn_validate: the validation head does not take this geometry (C=%d, %dx%d from "
              "%dx%d)", pl.net->num_classes, pl.H, pl.W, pl.H3, pl.W3);
    return E_UNSUPPORTED;
  }
  RunArgs r = forward_args(pl, x, x_dtype, params, running, nbt, ws, 0, 0.f, 0.1f, stream);
  r.validate = 1; r.target = target; r.ignore_index = ignore_index; r.loss2 = loss;
  r.head = head; r.smooth = smooth; r.dice_weight = dice_weight; r.focal_weight = focal_weight;
  r.alpha = alpha; r.gamma = gamma; r.aux_weight = aux_weight;
  r.counts = reinterpret_cast<unsigned long long*>(counts); r.head_ws = head_ws;
  GUARD(net_forward(plan->plan, r));
}

// ---- deployment pipeline (e2e.hip) -------------------------------------------------------------
static int e2e_pre_args(const void* x, int channels_last, int bgr, int N, int h, int w, int base,
                        const float* mean, const float* std, void* y, E2ePreArgs& a) {
  if (!x || !y) {
    set_error("fscnn_e2e_pre: null argument");
    return E_INVALID;
  }
  if ((mean == nullptr) != (std == nullptr)) {
    set_error("fscnn_e2e_pre: mean and std are given together or not at all");
    return E_INVALID;
  }
  a.x = x; a.y = y; a.N = N; a.h = h; a.w = w; a.base = base; a.bgr = bgr != 0;
  const long long hw = (long long)h * w;
  a.sn = 3 * hw;
  if (channels_last) { a.sc = 1; a.sy = 3LL * w; a.sx = 3; }
  else { a.sc = hw; a.sy = w; a.sx = 1; }
  for (int c = 0; c < 3; ++c) {
    if (mean && !(std[c] != 0.f)) {
      set_error("fscnn_e2e_pre: std[%d] is zero or NaN", c);
      return E_INVALID;
    }
    const double s = mean ? (double)std[c] : 1.0;
    a.A[c] = 1.0 / (255.0 * s);
    a.B[c] = mean ? -(double)mean[c] / s : 0.0;
  }
  return OK;
}

int fscnn_e2e_pre(const void* x, int x_dtype, int channels_last, int bgr, int N, int h, int w,
                  int base, const float* mean, const float* std, void* y, int y_dtype,
                  void* stream) {
  E2ePreArgs a{};
  if (int rc = e2e_pre_args(x, channels_last, bgr, N, h, w, base, mean, std, y, a)) return rc;
  return e2e_pre(a, x_dtype, y_dtype, S(stream));
}

int fscnn_e2e_head(const void* logits, int dtype, int N, int Hc, int Wc, int C, int ldx, int base,
                   int h_out, int w_out, int softmax, void* probs, int probs_dtype,
                   unsigned char* labels, int label_scale, void* stream) {
  if (!logits) {
    set_error("fscnn_e2e_head: null logits");
    return E_INVALID;
  }
  E2eHeadArgs a{};
  a.N = N; a.Hl = Hc; a.Wl = Wc; a.C = C; a.base = base; a.Ho = h_out; a.Wo = w_out;
  a.logits = logits; a.ldx = ldx; a.softmax = softmax != 0; a.probs = probs;
  a.probs_dtype = probs_dtype; a.labels = labels; a.label_scale = label_scale;
  return e2e_head(a, dtype, S(stream));
}

static long long e2e_x_offset(const Plan& pl) {  // the front end's output, behind the forward ws
  return ((long long)pl.ws_bytes + 255) / 256 * 256;
}

long long fscnn_e2e_ws_bytes(const fscnn_plan* plan) {
  if (!plan || plan->plan.train) {
    set_error("fscnn_e2e_ws_bytes: the deployment pipeline needs an inference plan (train=0)");
    return E_INVALID;
  }
  const Plan& pl = plan->plan;
  return e2e_x_offset(pl) + 3LL * pl.N * pl.H * pl.W * (pl.dtype == DT_F32 ? 4 : 2);
}

// fscnn_forward_e2e and fscnn_forward_e2e_bev: the front end, then the backbone ending in the tail
// that `r` names (its x is set here).  tail_ok: the tail's geometry check, made before anything
// is launched.
static int forward_e2e_run(const char* who, const fscnn_plan* plan, const void* x, int x_dtype,
                           int channels_last, int bgr, int h, int w, const float* mean,
                           const float* std, bool tail_ok, RunArgs& r, void* ws, void* stream) {
  const Plan& pl = plan->plan;
  if (pl.train || pl.H != pl.W) {
    set_error("%s: needs an inference plan (train=0) of a square input, got train=%d %dx%d", who,
              pl.train, pl.H, pl.W);
    return E_INVALID;
  }
  // FSCNN_E2E_FUSED=0 (read on every call: tests compare the two routes in one process) reports
  // every geometry as unsupported, which sends the caller down its unfused route
  if (!env_on("FSCNN_E2E_FUSED")) {
    set_error("%s: switched off (FSCNN_E2E_FUSED=0)", who);
    return E_UNSUPPORTED;
  }
  if (!tail_ok) {
    set_error("%s: the tail does not take this geometry (C=%d, %dx%d from base %d, low-res %dx%d)",
              who, pl.net->num_classes, r.e2e_ho, r.e2e_wo, pl.H, pl.H3, pl.W3);
    return E_UNSUPPORTED;
  }
  void* xin = (char*)ws + e2e_x_offset(pl);
  E2ePreArgs a{};
  if (int rc = e2e_pre_args(x, channels_last, bgr, pl.N, h, w, pl.H, mean, std, xin, a)) return rc;
  if (int rc = e2e_pre(a, x_dtype, pl.dtype, S(stream))) return rc;
  r.x = xin;
  GUARD(net_forward(plan->plan, r));
}

int fscnn_forward_e2e(const fscnn_plan* plan, const void* x, int x_dtype, int channels_last,
                      int bgr, int h, int w, const float* mean, const float* std, int h_out,
                      int w_out, int softmax, void* probs, int probs_dtype, unsigned char* labels,
                      int label_scale, const float* params, float* running, long long* nbt,
                      void* ws, void* stream) {
  if (!plan || !x || !params || !running || !ws || (!probs && !labels)) {
    set_error("fscnn_forward_e2e: null argument");
    return E_INVALID;
  }
  if (probs && (probs_dtype < DT_F32 || probs_dtype > DT_F16)) {
    set_error("fscnn_forward_e2e: probs dtype %d (0 fp32, 1 bf16, 2 fp16)", probs_dtype);
    return E_INVALID;
  }
  const Plan& pl = plan->plan;
  RunArgs r = forward_args(pl, nullptr, pl.dtype, params, running, nbt, ws, 0, 0.f, 0.1f, stream);
  r.e2e_ho = h_out; r.e2e_wo = w_out; r.e2e_softmax = softmax != 0; r.e2e_probs = probs;
  r.e2e_pdtype = probs_dtype; r.e2e_labels = labels; r.e2e_scale = label_scale;
  return forward_e2e_run("fscnn_forward_e2e", plan, x, x_dtype, channels_last, bgr, h, w, mean, std,
                         e2e_head_ok(pl.N, pl.net->num_classes, pl.H3, pl.W3, pl.H, h_out, w_out),
                         r, ws, stream);
}

// ---- bird's-eye tail (bev.hip) -------------------------------------------------------------------
static int bev_args(const char* who, const double* m, int Hb, int Wb, int min_width,
                    unsigned char* bev, int* rows, BevArgs& b) {
  if (!m || !rows) {
    set_error("%s: null argument", who);
    return E_INVALID;
  }
  b.Hb = Hb; b.Wb = Wb; b.min_width = min_width; b.bev = bev; b.rows = rows;
  for (int i = 0; i < 9; ++i) b.m[i] = m[i];
  return OK;
}

int fscnn_bev_mask(const unsigned char* mask, int N, int h, int w, const double* m, int Hb, int Wb,
                   int min_width, unsigned char* bev, int* rows, void* stream) {
  BevArgs b{};
  if (int rc = bev_args("fscnn_bev_mask", m, Hb, Wb, min_width, bev, rows, b)) return rc;
  b.N = N; b.Ho = h; b.Wo = w;
  return bev_mask(b, mask, S(stream));
}

int fscnn_e2e_bev(const void* logits, int dtype, int N, int Hc, int Wc, int C, int ldx, int base,
                  int h, int w, int label_scale, const double* m, int Hb, int Wb, int min_width,
                  unsigned char* bev, int* rows, void* stream) {
  BevArgs b{};
  if (int rc = bev_args("fscnn_e2e_bev", m, Hb, Wb, min_width, bev, rows, b)) return rc;
  E2eHeadArgs a{};
  a.N = N; a.Hl = Hc; a.Wl = Wc; a.C = C; a.base = base; a.Ho = h; a.Wo = w;
  a.logits = logits; a.ldx = ldx; a.label_scale = label_scale;
  return e2e_bev(a, b, dtype, S(stream));
}

int fscnn_forward_e2e_bev(const fscnn_plan* plan, const void* x, int x_dtype, int channels_last,
                          int bgr, int h, int w, const float* mean, const float* std, int h_out,
                          int w_out, int label_scale, const double* m, int Hb, int Wb,
                          int min_width, unsigned char* bev, int* rows, const float* params,
                          float* running, long long* nbt, void* ws, void* stream) {
  if (!plan || !x || !params || !running || !ws) {
    set_error("fscnn_forward_e2e_bev: null argument");
    return E_INVALID;
  }
  BevArgs b{};
  if (int rc = bev_args("fscnn_forward_e2e_bev", m, Hb, Wb, min_width, bev, rows, b)) return rc;
  for (int i = 0; i < 9; ++i)
    if (!std::isfinite(m[i])) {
      set_error("fscnn_forward_e2e_bev: m[%d] is not finite", i);
      return E_INVALID;
    }
  const Plan& pl = plan->plan;
  RunArgs r = forward_args(pl, nullptr, pl.dtype, params, running, nbt, ws, 0, 0.f, 0.1f, stream);
  r.e2e_ho = h_out; r.e2e_wo = w_out; r.e2e_scale = label_scale;
  r.bev_hb = Hb; r.bev_wb = Wb; r.bev_min_width = min_width; r.bev_mask = bev; r.bev_rows = rows;
  for (int i = 0; i < 9; ++i) r.bev_m[i] = m[i];
  return forward_e2e_run("fscnn_forward_e2e_bev", plan, x, x_dtype, channels_last, bgr, h, w, mean,
                         std, e2e_bev_ok(pl.N, pl.net->num_classes, pl.H3, pl.W3, pl.H, h_out,
                                         w_out, Hb, Wb, min_width),
                         r, ws, stream);
}

// ---- steering tail (path.hip) ----------------------------------------------------------------------
int fscnn_path_plan(const int* rows, int N, int Hb, const fscnn_path_params* p, double* ema_state,
                    double* out, void* stream) {
  if (!p) {
    set_error("fscnn_path_plan: null parameters");
    return E_INVALID;
  }
  return path_plan(rows, N, Hb, *p, ema_state, out, S(stream));
}

// ---- colour bird's-eye view (bev_image.hip) --------------------------------------------------------
int fscnn_bev_image(const unsigned char* frames, int channels_last, int N, int h, int w,
                    const double* m, int Hb, int Wb, unsigned char* image,
                    const unsigned char* bev_mask, const unsigned char* color, float frame_weight,
                    float alpha, float gamma, unsigned char* blended, void* stream) {
  if (!frames || !m) {
    set_error("fscnn_bev_image: null argument");
    return E_INVALID;
  }
  if (blended && (!bev_mask || !color)) {
    set_error("fscnn_bev_image: the blended output needs bev_mask and color");
    return E_INVALID;
  }
  BevImageArgs a{};
  a.frames = frames; a.channels_last = channels_last != 0; a.N = N; a.h = h; a.w = w;
  a.Hb = Hb; a.Wb = Wb; a.image = image; a.blended = blended;
  a.bev_mask = blended ? bev_mask : nullptr;
  for (int i = 0; i < 9; ++i) a.m[i] = m[i];
  for (int k = 0; k < 3; ++k) a.color[k] = blended ? color[k] : 0;
  a.frame_weight = frame_weight; a.alpha = alpha; a.gamma = gamma;
  return bev_image(a, S(stream));
}

// ---- overlay tail (overlay.hip) --------------------------------------------------------------------
static int overlay_args(const char* who, const void* frames, int frame_dtype, int channels_last,
                        int N, int h, int w, float frame_weight, float alpha, float gamma,
                        unsigned char* out, unsigned char* mask_out, OverlayArgs& o) {
  if (!frames || !out) {
    set_error("%s: null frames or out", who);
    return E_INVALID;
  }
  if (h < 2 || w < 2) {
    set_error("%s: frame %dx%d (sides >= 2)", who, h, w);
    return E_INVALID;
  }
  o.frames = frames; o.frame_dtype = frame_dtype; o.channels_last = channels_last != 0;
  o.N = N; o.h = h; o.w = w; o.frame_weight = frame_weight; o.alpha = alpha; o.gamma = gamma;
  o.out = out; o.mask_out = mask_out;
  return OK;
}

static int overlay_colors(const char* who, const unsigned char* colors, int C,
                          unsigned class_mask, OverlayColors& t) {
  if (!colors || C < 1) {
    set_error("%s: null colors or C=%d", who, C);
    return E_INVALID;
  }
  t = OverlayColors{};
  for (int c = 0; c < C && c < OV_CMAX; ++c)
    for (int k = 0; k < 3; ++k) t.c[c][k] = colors[c * 3 + k];
  t.on = class_mask;
  return OK;
}

int fscnn_overlay_mask(const void* frames, int frame_dtype, int channels_last, int N, int h, int w,
                       const unsigned char* mask, int Hm, int Wm, const unsigned char* color,
                       const unsigned char* palette, int P, float frame_weight, float alpha,
                       float gamma, unsigned char* out, unsigned char* mask_out, void* stream) {
  OverlayArgs o{};
  if (int rc = overlay_args("fscnn_overlay_mask", frames, frame_dtype, channels_last, N, h, w,
                            frame_weight, alpha, gamma, out, mask_out, o))
    return rc;
  if (!palette && !color) {
    set_error("fscnn_overlay_mask: neither a color nor a palette");
    return E_INVALID;
  }
  OverlayColors t{};
  if (!palette)
    for (int k = 0; k < 3; ++k) t.c[0][k] = color[k];
  return overlay_mask(o, mask, Hm, Wm, t, palette, P, S(stream));
}

int fscnn_e2e_overlay(const void* logits, int dtype, int N, int Hc, int Wc, int C, int ldx,
                      int base, int h_out, int w_out, int label_scale, const void* frames,
                      int frame_dtype, int channels_last, int h, int w,
                      const unsigned char* colors, unsigned class_mask, float frame_weight,
                      float alpha, float gamma, unsigned char* out, unsigned char* mask_out,
                      void* stream) {
  OverlayArgs o{};
  if (int rc = overlay_args("fscnn_e2e_overlay", frames, frame_dtype, channels_last, N, h, w,
                            frame_weight, alpha, gamma, out, mask_out, o))
    return rc;
  OverlayColors t{};
  if (int rc = overlay_colors("fscnn_e2e_overlay", colors, C, class_mask, t)) return rc;
  E2eHeadArgs a{};
  a.N = N; a.Hl = Hc; a.Wl = Wc; a.C = C; a.base = base; a.Ho = h_out; a.Wo = w_out;
  a.logits = logits; a.ldx = ldx; a.label_scale = label_scale;
  return e2e_overlay(a, o, t, dtype, S(stream));
}

int fscnn_forward_e2e_overlay(const fscnn_plan* plan, const void* x, int x_dtype,
                              int channels_last, int bgr, int h, int w, const float* mean,
                              const float* std, int h_out, int w_out, int label_scale,
                              const unsigned char* colors, unsigned class_mask,
                              float frame_weight, float alpha, float gamma, unsigned char* out,
                              unsigned char* mask_out, const float* params, float* running,
                              long long* nbt, void* ws, void* stream) {
  if (!plan || !x || !params || !running || !ws) {
    set_error("fscnn_forward_e2e_overlay: null argument");
    return E_INVALID;
  }
  const Plan& pl = plan->plan;
  RunArgs r = forward_args(pl, nullptr, pl.dtype, params, running, nbt, ws, 0, 0.f, 0.1f, stream);
  if (int rc = overlay_args("fscnn_forward_e2e_overlay", x, x_dtype, channels_last, pl.N, h, w,
                            frame_weight, alpha, gamma, out, mask_out, r.ov))
    return rc;
  if ((const void*)out == x || (const void*)mask_out == x || out == mask_out) {
    set_error("fscnn_forward_e2e_overlay: the outputs are fresh buffers; aliasing the frames is "
              "refused");
    return E_INVALID;
  }
  if (x_dtype < DT_F32 || x_dtype > DT_U8) {
    set_error("fscnn_forward_e2e_overlay: frame dtype %d (0 fp32, 1 bf16, 2 fp16, 3 uint8)",
              x_dtype);
    return E_INVALID;
  }
  if (int rc = overlay_colors("fscnn_forward_e2e_overlay", colors, pl.net->num_classes,
                              class_mask, r.ov_colors))
    return rc;
  r.e2e_ho = h_out; r.e2e_wo = w_out; r.e2e_scale = label_scale;
  return forward_e2e_run("fscnn_forward_e2e_overlay", plan, x, x_dtype, channels_last, bgr, h, w,
                         mean, std, e2e_overlay_ok(pl.N, pl.net->num_classes, pl.H3, pl.W3, pl.H,
                                                   h_out, w_out, h, w),
                         r, ws, stream);
}

int fscnn_seg_metric(const void* pred, int pred_dtype, const long long* target, long long n,
                     int nclass, long long* counts, void* stream) {
  if ((!pred || !target || !counts) && n > 0) {
    set_error("fscnn_seg_metric: null argument");
    return E_INVALID;
  }
  if (pred_dtype != 0 && pred_dtype != 1) {
    set_error("fscnn_seg_metric: pred_dtype %d (0 int64, 1 uint8)", pred_dtype);
    return E_INVALID;
  }
  return seg_metric(pred, pred_dtype, target, n, nclass, counts, S(stream));
}

int fscnn_normalize_u8(const unsigned char* images, int N, int H, int W, const float* mean,
                       const float* std, void* out, int out_dtype, void* stream) {
  if (!images || !mean || !std || !out) {
    set_error("fscnn_normalize_u8: null argument");
    return E_INVALID;
  }
  if (out_dtype != DT_F32 && out_dtype != DT_BF16) {
    set_error("fscnn_normalize_u8: out_dtype %d", out_dtype);
    return E_INVALID;
  }
  return normalize_u8(images, N, H, W, mean, std, out, out_dtype, S(stream));
}

int fscnn_remap_labels(const unsigned char* labels, long long n, const long long* lut, int lut_size,
                       int offset, long long invalid, long long* out, void* stream) {
  if ((!labels || !out || !lut) && n > 0) {
    set_error("fscnn_remap_labels: null argument");
    return E_INVALID;
  }
  return remap_labels(labels, n, lut, lut_size, offset, invalid, out, S(stream));
}

int fscnn_sync_tables(int in_size, int out_size, int start, int count, int kmax, int* bounds,
                      int* coef, int* nearest, int* ksize) {
  return sync_tables(in_size, out_size, start, count, kmax, bounds, coef, nearest, ksize);
}

int fscnn_sync_blur_weights(float radius, unsigned* ww, unsigned* fw) {
  return sync_blur_weights(radius, ww, fw);
}

int fscnn_sync_transform(const void* host_blob, const void* device_blob, long long blob_bytes,
                         int N, int crop, const long long* lut, int lut_size, int lut_offset,
                         const float* mean, const float* std, void* x, int out_dtype,
                         long long* target, unsigned char* crop_u8, void* stream) {
  if (!host_blob || !device_blob || !lut || !mean || !std || !x || !target) {
    set_error("fscnn_sync_transform: null argument");
    return E_INVALID;
  }
  if (out_dtype != DT_F32 && out_dtype != DT_BF16) {
    set_error("fscnn_sync_transform: out_dtype %d", out_dtype);
    return E_INVALID;
  }
  return sync_transform(host_blob, device_blob, blob_bytes, N, crop, lut, lut_size, lut_offset,
                        mean, std, x, out_dtype, target, crop_u8, S(stream));
}

int fscnn_ohem_prob(const void* logits, int dtype, const long long* target, int N, int C,
                    long long HW, long long ignore_index, float thresh, float* prob,
                    unsigned long long* counts, void* stream) {
  if (!logits || !target || !prob || !counts) {
    set_error("fscnn_ohem_prob: null argument");
    return E_INVALID;
  }
  CeArgs a{};
  a.N = N; a.C = C; a.HW = HW; a.logits = logits; a.target = target; a.ignore_index = ignore_index;
  return ohem_prob(a, thresh, prob, counts, dtype, S(stream));
}

int fscnn_ohem_threshold(const float* prob, long long n, const unsigned long long* counts,
                         long long min_kept, float thresh, unsigned* work, float* thr, void* stream) {
  if (!prob || !counts || !work || !thr) {
    set_error("fscnn_ohem_threshold: null argument");
    return E_INVALID;
  }
  return ohem_threshold_dev(prob, n, counts, min_kept, thresh, work, thr, S(stream));
}

int fscnn_kth_smallest(const float*, long long, long long, unsigned*, float*, void*) {
  set_error("fscnn_kth_smallest was removed in round 3: use fscnn_ohem_threshold (the whole OHEM "
            "threshold rule on the device, no host sync)");
  return E_UNSUPPORTED;
}

int fscnn_ce_weighted_fwd(const void* logits, int dtype, const long long* target, int N, int C,
                          long long HW, long long ignore_index, const float* weight,
                          const float* prob, const float* thr, float* part, float* out2,
                          void* stream) {
  if (prob && !thr) {
    set_error("fscnn_ce_weighted_fwd: prob without thr");
    return E_INVALID;
  }
  CeArgs a{};
  a.N = N; a.C = C; a.HW = HW; a.logits = logits; a.target = target;
  a.ignore_index = ignore_index; a.part = part; a.weight = weight; a.prob = prob; a.thr = thr;
  return ce_fwd(a, out2, dtype, S(stream));
}

int fscnn_ce_weighted_bwd(const void* logits, int dtype, const long long* target, int N, int C,
                          long long HW, long long ignore_index, const float* weight,
                          const float* prob, const float* thr, const float* grad_out,
                          const float* out2, void* dlogits, void* stream) {
  if (prob && !thr) {
    set_error("fscnn_ce_weighted_bwd: prob without thr");
    return E_INVALID;
  }
  CeArgs a{};
  a.N = N; a.C = C; a.HW = HW; a.logits = logits; a.target = target;
  a.ignore_index = ignore_index; a.dlogits = dlogits; a.weight = weight; a.prob = prob; a.thr = thr;
  return ce_bwd(a, grad_out, out2, dtype, S(stream));
}

int fscnn_dice_fwd(const void* logits, int dtype, const long long* target, int N, int C,
                   long long HW, float alpha, float gamma, int focal, float* part, double* stats,
                   void* stream) {
  if (!logits || !target || !part || !stats) {
    set_error("fscnn_dice_fwd: null argument");
    return E_INVALID;
  }
  return dice_loss_fwd(logits, dtype, target, N, C, HW, alpha, gamma, focal, part, stats, S(stream));
}

int fscnn_dice_bwd(const void* logits, int dtype, const long long* target, int N, int C,
                   long long HW, float alpha, float gamma, int focal, const double* stats,
                   const float* grad_out, float smooth, float dice_weight, float focal_weight,
                   void* dlogits, void* stream) {
  if (!logits || !target || !stats || !grad_out || !dlogits) {
    set_error("fscnn_dice_bwd: null argument");
    return E_INVALID;
  }
  return dice_loss_bwd(logits, dtype, target, N, C, HW, alpha, gamma, focal, stats, grad_out,
                       smooth, dice_weight, focal_weight, dlogits, S(stream));
}

int fscnn_forward_loss(const fscnn_plan* plan, const void* x, int x_dtype, const long long* target,
                       long long ignore_index, float* loss2, const float* params, float* running,
                       long long* nbt, void* ws, unsigned long long seed, float dropout_p,
                       float momentum, void* stream) {
  if (!plan || !x || !target || !loss2 || !params || !running || !ws) {
    set_error("fscnn_forward_loss: null argument");
    return E_INVALID;
  }
  RunArgs r = forward_args(plan->plan, x, x_dtype, params, running, nbt, ws, seed, dropout_p,
                           momentum, stream);
  r.target = target; r.ignore_index = ignore_index; r.loss2 = loss2;
  GUARD(net_forward(plan->plan, r));
}

int fscnn_backward_loss(const fscnn_plan* plan, const float* grad_loss, const float* loss2,
                        const void* x, int x_dtype, const float* params, float* grads, void* ws,
                        void* bws, unsigned long long seed, float dropout_p, int stage_from,
                        int stage_to, void* stream) {
  if (!plan || !grad_loss || !loss2 || !x || !params || !grads || !ws || !bws) {
    set_error("fscnn_backward_loss: null argument");
    return E_INVALID;
  }
  RunArgs r = backward_args(x, x_dtype, params, grads, ws, bws, seed, dropout_p, stream);
  r.gloss = grad_loss; r.loss2 = const_cast<float*>(loss2);
  GUARD(net_backward(plan->plan, r, stage_from, stage_to));
}

long long fscnn_dice_head_ws_bytes(const fscnn_plan* plan) {
  if (!plan || plan->plan.train != 1) {
    set_error("fscnn_dice_head_ws_bytes: the fused loss head needs a training plan (train=1)");
    return E_INVALID;
  }
  const Plan& pl = plan->plan;
  return dice_head_ws_bytes(pl.N, pl.H3, pl.W3, pl.net->num_classes, pl.Cp);
}

int fscnn_forward_loss_dice(const fscnn_plan* plan, const void* x, int x_dtype,
                            const long long* target, float smooth, float dice_weight,
                            float focal_weight, float alpha, float gamma, float* loss_out,
                            double* stats, const float* params, float* running, long long* nbt,
                            void* ws, void* head_ws, unsigned long long seed, float dropout_p,
                            float momentum, void* stream) {
  if (!plan || !x || !target || !loss_out || !stats || !params || !running || !ws || !head_ws) {
    set_error("fscnn_forward_loss_dice: null argument");
    return E_INVALID;
  }
  RunArgs r = forward_args(plan->plan, x, x_dtype, params, running, nbt, ws, seed, dropout_p,
                           momentum, stream);
  r.target = target; r.ignore_index = -1; r.loss2 = loss_out;
  r.head = HEAD_DICE; r.smooth = smooth; r.dice_weight = dice_weight;
  r.focal_weight = focal_weight; r.alpha = alpha; r.gamma = gamma;
  r.head_ws = head_ws; r.dice_stats = stats;
  GUARD(net_forward(plan->plan, r));
}

int fscnn_backward_loss_dice(const fscnn_plan* plan, const float* grad_loss, const double* stats,
                             float smooth, float dice_weight, float focal_weight, const void* x,
                             int x_dtype, const float* params, float* grads, void* ws, void* bws,
                             void* head_ws, unsigned long long seed, float dropout_p,
                             int stage_from, int stage_to, void* stream) {
  if (!plan || !grad_loss || !stats || !x || !params || !grads || !ws || !bws || !head_ws) {
    set_error("fscnn_backward_loss_dice: null argument");
    return E_INVALID;
  }
  if (plan->plan.net->aux) {
    set_error("backward_loss: the fused loss head covers the main output only (aux net)");
    return E_UNSUPPORTED;
  }
  RunArgs r = backward_args(x, x_dtype, params, grads, ws, bws, seed, dropout_p, stream);
  r.gloss = grad_loss;
  r.head = HEAD_DICE; r.smooth = smooth; r.dice_weight = dice_weight;
  r.focal_weight = focal_weight; r.head_ws = head_ws; r.dice_stats = const_cast<double*>(stats);
  GUARD(net_backward(plan->plan, r, stage_from, stage_to));
}

int fscnn_forward_loss_ohem(const fscnn_plan* plan, const void* x, int x_dtype,
                            const long long* target, long long ignore_index, float thresh,
                            long long min_kept, const float* weight, float* loss2, float* prob,
                            float* thr, unsigned long long* counts, unsigned* work,
                            const float* params, float* running, long long* nbt, void* ws,
                            unsigned long long seed, float dropout_p, float momentum,
                            void* stream) {
  if (!plan || !x || !target || !loss2 || !prob || !thr || !counts || !work || !params ||
      !running || !ws) {
    set_error("fscnn_forward_loss_ohem: null argument");
    return E_INVALID;
  }
  if (min_kept < 0) {
    set_error("fscnn_forward_loss_ohem: min_kept=%lld", min_kept);
    return E_INVALID;
  }
  // refusals come before anything is launched
  if (plan->plan.net->aux) {
    set_error("forward_loss: the fused loss head covers the main output only (aux net)");
    return E_UNSUPPORTED;
  }
  if (!ohem_head_ok(plan->plan.net->num_classes)) {
    set_error("fscnn_forward_loss_ohem: %d classes (the fused OHEM head takes 1 .. 32)",
              plan->plan.net->num_classes);
    return E_UNSUPPORTED;
  }
  RunArgs r = forward_args(plan->plan, x, x_dtype, params, running, nbt, ws, seed, dropout_p,
                           momentum, stream);
  r.target = target; r.ignore_index = ignore_index; r.loss2 = loss2;
  r.head = HEAD_OHEM; r.ohem_thresh = thresh; r.ohem_min_kept = min_kept;
  r.ohem_weight = weight; r.ohem_prob = prob; r.ohem_thr = thr; r.ohem_counts = counts;
  r.ohem_work = work;
  GUARD(net_forward(plan->plan, r));
}

long long fscnn_aux_head_ws_bytes(const fscnn_plan* plan, int head) {
  if (!plan) {
    set_error("fscnn_aux_head_ws_bytes: null plan");
    return E_INVALID;
  }
  AuxHeadWs l;
  if (!aux_head_ws(plan->plan, head, l)) return E_INVALID;
  return (long long)l.bytes;
}

long long fscnn_aux_head_ws_offset(const fscnn_plan* plan, int head, const char* field, int which) {
  if (!plan || !field || which < 0 || which > 1) {
    set_error("fscnn_aux_head_ws_offset: null argument / which=%d", which);
    return E_INVALID;
  }
  AuxHeadWs l;
  if (!aux_head_ws(plan->plan, head, l)) return E_INVALID;
  const std::string f = field;
  const bool ohem = head == HEAD_OHEM, dice = head == HEAD_DICE;
  if (f == "pair") return (long long)l.pair[which];
  if (f == "stats" && dice) return (long long)l.stats[which];
  if (f == "prob" && ohem) return (long long)l.prob[which];
  if (f == "thr" && ohem) return (long long)l.thr[which];
  if (f == "counts" && ohem) return (long long)l.counts[which];
  set_error("fscnn_aux_head_ws_offset: head %d has no field '%s'", head, field);
  return E_INVALID;
}

// the checks both aux loss entries share (after the null checks, before anything is launched),
// and the head's fields of RunArgs
static int aux_head_args(const char* who, const fscnn_plan* plan, const fscnn_aux_head* h,
                         RunArgs& r) {
  AuxHeadWs l;
  if (!aux_head_ws(plan->plan, h->head, l)) {
    const std::string why = fscnn_last_error();
    set_error("%s: %s", who, why.c_str());
    return E_INVALID;
  }
  if (h->head == HEAD_OHEM && h->min_kept < 0) {
    set_error("%s: min_kept=%lld", who, h->min_kept);
    return E_INVALID;
  }
  const int C = plan->plan.net->num_classes;
  if (!ohem_head_ok(C) || (h->head == HEAD_DICE && C < 2)) {
    set_error("%s: %d classes (the fused heads take 1 .. 32, the Dice head from 2)", who, C);
    return E_UNSUPPORTED;
  }
  if (h->head == HEAD_DICE && h->focal_weight != 0.f) {
    set_error("%s: focal_weight=%g (the aux Dice head is plain Dice: the reference has no "
              "two-output Focal+Dice criterion)", who, h->focal_weight);
    return E_UNSUPPORTED;
  }
  r.aux_loss = 1; r.head = h->head; r.aux_weight = h->aux_weight;
  r.ignore_index = h->head == HEAD_DICE ? -1 : h->ignore_index;
  if (h->head == HEAD_DICE) {
    r.smooth = h->smooth; r.dice_weight = h->dice_weight; r.focal_weight = h->focal_weight;
    r.alpha = h->alpha; r.gamma = h->gamma;
  }
  if (h->head == HEAD_OHEM) {
    r.ohem_thresh = h->thresh; r.ohem_min_kept = h->min_kept; r.ohem_weight = h->class_weight;
  }
  return OK;
}

int fscnn_forward_loss_aux(const fscnn_plan* plan, const void* x, int x_dtype,
                           const long long* target, const fscnn_aux_head* h, float* loss_out,
                           const float* params, float* running, long long* nbt, void* ws,
                           void* head_ws, unsigned long long seed, float dropout_p, float momentum,
                           void* stream) {
  if (!plan || !x || !target || !h || !loss_out || !params || !running || !ws || !head_ws) {
    set_error("fscnn_forward_loss_aux: null argument");
    return E_INVALID;
  }
  RunArgs r = forward_args(plan->plan, x, x_dtype, params, running, nbt, ws, seed, dropout_p,
                           momentum, stream);
  if (int rc = aux_head_args("fscnn_forward_loss_aux", plan, h, r)) return rc;
  r.target = target; r.loss3 = loss_out; r.head_ws = head_ws;
  GUARD(net_forward(plan->plan, r));
}

int fscnn_backward_loss_aux(const fscnn_plan* plan, const float* grad_loss,
                            const fscnn_aux_head* h, const void* x, int x_dtype, void* dx,
                            int dx_dtype, const float* params, float* grads, void* ws, void* bws,
                            void* head_ws, unsigned long long seed, float dropout_p,
                            int stage_from, int stage_to, void* stream) {
  if (!plan || !grad_loss || !h || !x || !params || !grads || !ws || !bws || !head_ws) {
    set_error("fscnn_backward_loss_aux: null argument");
    return E_INVALID;
  }
  RunArgs r = backward_args(x, x_dtype, params, grads, ws, bws, seed, dropout_p, stream);
  if (int rc = aux_head_args("fscnn_backward_loss_aux", plan, h, r)) return rc;
  if (dx && h->head == HEAD_DICE) {
    set_error("fscnn_backward_loss_aux: the Dice head does not form the input gradient");
    return E_INVALID;
  }
  r.gloss = grad_loss; r.head_ws = head_ws; r.dx = dx; r.dx_dtype = dx_dtype;
  GUARD(net_backward(plan->plan, r, stage_from, stage_to));
}

int fscnn_backward_dx(const fscnn_plan* plan, const void* dout, const void* daux,
                      const float* grad_loss, const float* loss2, const void* x, int x_dtype,
                      void* dx, int dx_dtype, const float* params, float* grads, void* ws,
                      void* bws, unsigned long long seed, float dropout_p, int stage_from,
                      int stage_to, void* stream) {
  if (!plan || !x || !params || !grads || !ws || !bws || (!dout && !grad_loss) ||
      (dout && grad_loss) || (grad_loss && !loss2)) {
    set_error("fscnn_backward_dx: null argument (exactly one of dout / grad_loss + loss2)");
    return E_INVALID;
  }
  RunArgs r = backward_args(x, x_dtype, params, grads, ws, bws, seed, dropout_p, stream);
  r.dout = dout; r.daux = daux; r.gloss = grad_loss; r.loss2 = const_cast<float*>(loss2);
  r.dx = dx; r.dx_dtype = dx_dtype;
  GUARD(net_backward(plan->plan, r, stage_from, stage_to));
}

long long fscnn_ce_parts(int N, long long HW) { return ce_parts(N, HW); }

int fscnn_ce_fwd(const void* logits, int dtype, const long long* target, int N, int C,
                 long long HW, long long ignore_index, float* part, float* out2, void* stream) {
  CeArgs a{};
  a.N = N; a.C = C; a.HW = HW; a.logits = logits; a.target = target;
  a.ignore_index = ignore_index; a.part = part;
  return ce_fwd(a, out2, dtype, S(stream));
}
int fscnn_ce_bwd(const void* logits, int dtype, const long long* target, int N, int C,
                 long long HW, long long ignore_index, const float* grad_out, const float* out2,
                 void* dlogits, void* stream) {
  CeArgs a{};
  a.N = N; a.C = C; a.HW = HW; a.logits = logits; a.target = target;
  a.ignore_index = ignore_index; a.dlogits = dlogits;
  return ce_bwd(a, grad_out, out2, dtype, S(stream));
}
int fscnn_sgd(float* p, const float* g, float* buf, long long n, float lr, float momentum,
              float dampening, float weight_decay, int nesterov, int first, float grad_scale,
              void* stream) {
  SgdArgs a{};
  a.n = n; a.p = p; a.g = g; a.buf = buf; a.lr = lr; a.momentum = momentum;
  a.dampening = dampening; a.weight_decay = weight_decay; a.nesterov = nesterov; a.first = first;
  a.grad_scale = grad_scale;
  return sgd(a, S(stream));
}
int fscnn_adamw(float* p, const float* g, float* exp_avg, float* exp_avg_sq,
                float* max_exp_avg_sq, long long n, double lr, double beta1, double beta2,
                double eps, double weight_decay, int amsgrad, int maximize, float* step, int tick,
                const float* grad_scale, const float* found_inf, void* stream) {
  AdamwArgs a{};
  a.n = n; a.p = p; a.g = g; a.m = exp_avg; a.v = exp_avg_sq; a.vmax = max_exp_avg_sq;
  a.h = adamw_hyper(lr, beta1, beta2, eps, weight_decay, amsgrad, maximize, 0);
  a.step = step; a.tick = tick; a.grad_scale = grad_scale; a.found_inf = found_inf;
  return adamw(a, S(stream));
}
static_assert(sizeof(fscnn_adamw_seg) == sizeof(AdamwSeg) && FSCNN_ADAMW_CHUNK == ADAMW_CHUNK &&
              FSCNN_ADAMW_MAX_GROUPS == ADAMW_MAXGROUPS, "fastscnn.h and kernels.hpp disagree");
int fscnn_adamw_segments(float* p, const float* g, float* exp_avg, float* exp_avg_sq,
                         float* max_exp_avg_sq, const fscnn_adamw_seg* segs,
                         const fscnn_adamw_seg* host_segs, int nseg, const int* chunk_seg,
                         int nchunks, const fscnn_adamw_group* groups, int ngroups, float* steps,
                         int nslots, int tick, const float* grad_scale, const float* found_inf,
                         void* stream) {
  if (ngroups < 1 || ngroups > ADAMW_MAXGROUPS || !groups) {
    set_error("fscnn_adamw_segments: %d groups (1..%d per launch)", ngroups, ADAMW_MAXGROUPS);
    return E_INVALID;
  }
  AdamwSegArgs a{};
  a.p = p; a.g = g; a.m = exp_avg; a.v = exp_avg_sq; a.vmax = max_exp_avg_sq;
  a.segs = reinterpret_cast<const AdamwSeg*>(segs); a.chunk_seg = chunk_seg;
  a.nseg = nseg; a.nchunks = nchunks; a.ngroups = ngroups;
  for (int k = 0; k < ngroups; ++k) {
    const fscnn_adamw_group& g = groups[k];
    a.h[k] = adamw_hyper(g.lr, g.beta1, g.beta2, g.eps, g.weight_decay, g.amsgrad, g.maximize,
                         g.step_slot);
  }
  a.steps = steps; a.nslots = nslots; a.tick = tick;
  a.grad_scale = grad_scale; a.found_inf = found_inf;
  return adamw_segments(a, reinterpret_cast<const AdamwSeg*>(host_segs), S(stream));
}

int fscnn_conv0_fwd(const void* x, int x_dtype, int N, int H, int W, const float* w,
                    const float* scale, const float* shift, int relu, void* y, int y_dtype,
                    void* stream) {
  Conv0Args a{};
  a.x = x; a.x_bf16 = x_dtype; a.N = N; a.H = H; a.W = W;
  a.Ho = (H - 3) / 2 + 1; a.Wo = (W - 3) / 2 + 1; a.w = w; a.scale = scale; a.shift = shift;
  a.relu = relu; a.y = y;
  return conv0_fwd(a, y_dtype, S(stream));
}

long long fscnn_conv0_wgrad_slab_floats(int N, int H, int W) {
  return (long long)conv0_wgrad_parts(N, (H - 3) / 2 + 1, (W - 3) / 2 + 1, 0) * 864;
}
int fscnn_conv0_wgrad(const void* x, int x_dtype, int N, int H, int W, const void* dz,
                      int dz_dtype, float* slab, float* dw, void* stream) {
  Conv0WgradArgs a{};
  a.x = x; a.x_bf16 = x_dtype; a.N = N; a.H = H; a.W = W;
  a.Ho = (H - 3) / 2 + 1; a.Wo = (W - 3) / 2 + 1; a.dz = dz; a.slab = slab;
  int rc = conv0_wgrad(a, dz_dtype, S(stream));
  if (rc) return rc;
  return reduce_slabs(slab, conv0_wgrad_parts(N, a.Ho, a.Wo, 0), 864, 864, dw, 0, S(stream));
}

int fscnn_dw3x3_fwd(const void* x, int dtype, int N, int H, int W, int C, int stride,
                    const float* w, const float* scale, const float* shift, int relu, void* y,
                    void* stream) {
  DwArgs a{};
  a.N = N; a.H = H; a.W = W; a.C = C; a.stride = stride;
  a.Ho = (H - 1) / stride + 1; a.Wo = (W - 1) / stride + 1;
  a.x = x; a.w = w; a.scale = scale; a.shift = shift; a.relu = relu; a.y = y;
  return dw_fwd(a, dtype, S(stream));
}
int fscnn_dw3x3_dgrad(const void* dy, int dtype, int N, int H, int W, int C, int stride,
                      const float* w, void* dx, void* stream) {
  DwBwdArgs a{};
  a.N = N; a.H = H; a.W = W; a.C = C; a.stride = stride;
  a.Ho = (H - 1) / stride + 1; a.Wo = (W - 1) / stride + 1;
  a.dy = dy; a.w = w; a.dx = dx;
  return dw_dgrad(a, dtype, S(stream));
}
long long fscnn_dw3x3_wgrad_slab_floats(int N, int H, int W, int C, int stride, int dtype) {
  int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  return (long long)dw_wgrad_parts(N, Ho, Wo, C, dtype, stride) * 9 * C;
}
int fscnn_dw3x3_wgrad(const void* x, const void* dy, int dtype, int N, int H, int W, int C,
                      int stride, float* slab, float* dw, void* stream) {
  DwBwdArgs a{};
  a.N = N; a.H = H; a.W = W; a.C = C; a.stride = stride;
  a.Ho = (H - 1) / stride + 1; a.Wo = (W - 1) / stride + 1;
  a.x = x; a.dy = dy; a.slab = slab;
  int rc = dw_wgrad(a, dtype, S(stream));
  if (rc) return rc;
  return dw_wgrad_reduce(slab, dw_wgrad_parts(N, a.Ho, a.Wo, C, dtype, stride), C, dw, S(stream));
}

int fscnn_pw_gemm_stats_parts(int M, int N, int K, int lda, int ldc, int dtype) {
  GemmArgs a{};
  static float dummy;  // only the presence of the statistics pointer matters
  a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldb = K; a.ldc = ldc; a.part = &dummy;
  return gemm_nt_parts(a, dtype);
}
int fscnn_pw_gemm(int M, int N, int K, const void* A, int lda, const void* B, int ldb,
                  int b_trans, const float* scale, const float* shift, const void* R, int ldr,
                  int relu, void* C, int ldc, float* stats_part, int dtype, void* stream) {
  GemmArgs a{};
  a.M = M; a.N = N; a.K = K; a.A = A; a.lda = lda; a.B = B; a.ldb = ldb; a.b_trans = b_trans;
  a.scale = scale; a.shift = shift; a.R = R; a.ldr = ldr; a.relu = relu; a.C = C; a.ldc = ldc;
  a.part = stats_part;
  return gemm_nt(a, dtype, S(stream));
}
int fscnn_pw_dgrad_bnbwd(int M, int N, int K, const void* D, int ldd, const void* B, int ldb,
                         const void* R, int ldr, void* dX, int lddx, const void* z, int ldz,
                         const float* mean, const float* invstd, const float* scale,
                         const float* shift, int relu_mode, float* part, unsigned* counters,
                         double* tsum, float* dgamma, float* dbeta, float* coef, int dtype,
                         int* path, void* stream) {
  if (!D || !B || !dX || !z || !mean || !invstd || !scale || !shift || !part || !counters ||
      !tsum || !dgamma || !dbeta || !coef) {
    set_error("fscnn_pw_dgrad_bnbwd: null argument");
    return E_INVALID;
  }
  if (dtype < DT_F32 || dtype > DT_F16 || (relu_mode != 0 && relu_mode != 2)) {
    set_error("fscnn_pw_dgrad_bnbwd: dtype %d / relu_mode %d", dtype, relu_mode);
    return E_INVALID;
  }
  // the executor's form (net.cpp Exec::pw_bwd + set_btarget)
  GemmArgs a{};
  a.M = M; a.N = N; a.K = K; a.A = D; a.lda = ldd; a.B = B; a.ldb = ldb; a.b_trans = 0;
  a.R = R; a.ldr = ldr; a.C = dX; a.ldc = lddx;
  a.bpart = part; a.bz = z; a.ldbz = ldz;
  a.bmean = mean; a.binvstd = invstd; a.bscale = scale; a.bshift = shift; a.bmode = relu_mode;
  a.tail.counters = counters; a.tail.tsum = tsum; a.tail.count = (double)M;
  a.tail.dgamma = dgamma; a.tail.dbeta = dbeta; a.tail.coef = coef;
  if (path) *path = gemm_stream_ok(a, dtype) ? 1 : 0;
  return gemm_nt(a, dtype, S(stream));
}
long long fscnn_pw_wgrad_slab_floats(int M, int N, int K) {
  return (long long)gemm_tn_splits(M, N, K) * N * K;
}
int fscnn_pw_wgrad(int M, int N, int K, const void* D, int ldd, const void* X, int ldx,
                   float* slab, float* dW, int dtype, void* stream) {
  GemmTnArgs a{};
  a.M = M; a.N = N; a.K = K; a.D = D; a.ldd = ldd; a.X = X; a.ldx = ldx; a.slab = slab;
  int s = gemm_tn_splits(M, N, K);
  int rc = gemm_tn(a, s, dtype, S(stream));
  if (rc) return rc;
  return reduce_slabs(slab, s, (long long)N * K, (long long)N * K, dW, 0, S(stream));
}

int fscnn_bn_finalize(float* part, int P, int C, const float* gamma, const float* beta,
                      float* rmean, float* rvar, long long* nbt, float momentum, float* mean,
                      float* invstd, float* scale, float* shift, void* stream) {
  BnFinalizeArgs a{};
  a.part = part; a.P = P; a.C = C; a.gamma = gamma; a.beta = beta; a.rmean = rmean;
  a.rvar = rvar; a.nbt = nbt; a.momentum = momentum; a.mean = mean; a.invstd = invstd;
  a.scale = scale; a.shift = shift;
  return bn_finalize(a, S(stream));
}

int fscnn_bilinear_ac_fwd(const void* x, int dtype, int N, int Hi, int Wi, int C, int Ho, int Wo,
                          void* y, int out_nchw, int out_dtype, void* stream) {
  UpArgs a{};
  a.N = N; a.Hi = Hi; a.Wi = Wi; a.C = C; a.Ho = Ho; a.Wo = Wo; a.x = x; a.ldx = C; a.y = y;
  a.ldy = C;
  if (out_nchw) return up_nchw(a, dtype, out_dtype, S(stream));
  return up_nhwc(a, dtype, S(stream));
}
int fscnn_bilinear_ac_bwd(const void* dy, int dtype, int N, int Hi, int Wi, int C, int Ho, int Wo,
                          float* tmp, void* dx, void* stream) {
  AxisBwdArgs a{};
  a.n_o1 = (long long)N * Ho; a.n_o2 = 1; a.Lout = Wo; a.Lin = Wi; a.n_in = C;
  a.g = dy; a.g_s1 = (long long)Wo * C; a.g_idx = C; a.g_in = 1;
  a.d = tmp; a.d_s1 = (long long)Wi * C; a.d_idx = C; a.d_in = 1;
  int rc = axis_bwd(a, dtype, DT_F32, S(stream));
  if (rc) return rc;
  AxisBwdArgs b{};
  b.n_o1 = N; b.n_o2 = 1; b.Lout = Ho; b.Lin = Hi; b.n_in = (long long)Wi * C;
  b.g = tmp; b.g_s1 = (long long)Ho * Wi * C; b.g_idx = (long long)Wi * C; b.g_in = 1;
  b.d = dx; b.d_s1 = (long long)Hi * Wi * C; b.d_idx = (long long)Wi * C; b.d_in = 1;
  return axis_bwd(b, DT_F32, dtype, S(stream));
}
int fscnn_pyramid_pool_fwd(const void* x, int dtype, int N, int H, int W, int C, int ldx,
                           void* pooled, void* stream) {
  PoolArgs a{};
  a.N = N; a.H = H; a.W = W; a.C = C; a.x = x; a.ldx = ldx; a.pooled = pooled;
  return pyramid_pool(a, dtype, S(stream));
}
int fscnn_pyramid_pool_bwd(const void* dpooled, int dtype, int N, int H, int W, int C, void* dx,
                           int lddx, int accumulate, void* stream) {
  PoolBwdArgs a{};
  a.N = N; a.H = H; a.W = W; a.C = C; a.dpooled = dpooled; a.dx = dx; a.lddx = lddx;
  a.accumulate = accumulate;
  return pyramid_pool_bwd(a, dtype, S(stream));
}

// ---- the kernels only a train step runs, in the executor's form (tests/test_gpu_train_kernels.py).
// Each wrapper fills the *Args struct as net.cpp does and refuses null / inconsistent arguments
// before anything is launched; none has arithmetic of its own.
static bool dt_ok(int dtype) { return dtype >= DT_F32 && dtype <= DT_F16; }
static int vec_w(int dtype) { return dtype == DT_F32 ? 4 : 8; }  // elements per 16-B vector
// a row stride the 16-B vector loads take: >= C and a multiple of the vector width
static bool ld_ok(int ld, int C, int V) { return ld >= C && ld % V == 0; }

int fscnn_bn_apply(long long M, int C, const void* z, int ldz, const float* scale,
                   const float* shift, const void* z2, int ldz2, const float* scale2,
                   const float* shift2, const void* res, int ldres, int relu, void* y, int ldy,
                   int dtype, void* stream) {
  if (!z || !scale || !shift || !y || (z2 && (!scale2 || !shift2))) {
    set_error("fscnn_bn_apply: null argument");
    return E_INVALID;
  }
  if (!dt_ok(dtype)) {
    set_error("fscnn_bn_apply: dtype %d", dtype);
    return E_INVALID;
  }
  const int V = vec_w(dtype);
  if (M < 1 || C < 1 || C % V || !ld_ok(ldz, C, V) || !ld_ok(ldy, C, V) ||
      (z2 && !ld_ok(ldz2, C, V)) || (res && !ld_ok(ldres, C, V)) ||
      M * (C / V) >= (1LL << 31)) {
    set_error("fscnn_bn_apply: M=%lld C=%d ldz=%d ldz2=%d ldres=%d ldy=%d (C and every row stride "
              "a multiple of %d, strides >= C)", M, C, ldz, ldz2, ldres, ldy, V);
    return E_INVALID;
  }
  // net.cpp Exec::apply (plain / residual) and the FFM's two-branch form
  BnApplyArgs a{};
  a.M = M; a.C = C;
  a.z = z; a.ldz = ldz; a.scale = scale; a.shift = shift;
  a.z2 = z2; a.ldz2 = ldz2; a.scale2 = scale2; a.shift2 = shift2;
  a.res = res; a.ldres = ldres;
  a.relu = relu;
  a.y = y; a.ldy = ldy;
  return bn_apply(a, dtype, S(stream));
}

int fscnn_bn_bwd(long long M, int C, const void* dy, int lddy, const void* mask, int ldmask,
                 const void* z, const float* mean, const float* invstd, const float* scale,
                 const float* shift, int relu_mode, int frozen, const void* z2,
                 const float* mean2, const float* invstd2, const float* scale2, float* part,
                 unsigned* counters, void* dz, void* dz2, float* dgamma, float* dbeta,
                 float* dgamma2, float* dbeta2, float* coef, int dtype, int* P_out,
                 int* rows_per_block_out, void* stream) {
  if (!dy || !z || !mean || !invstd || !scale || !part || !counters || !dz || !dgamma || !dbeta ||
      !coef) {
    set_error("fscnn_bn_bwd: null argument");
    return E_INVALID;
  }
  if (!dt_ok(dtype) || relu_mode < 0 || relu_mode > 2 || frozen < 0 || frozen > 2) {
    set_error("fscnn_bn_bwd: dtype %d / relu_mode %d / frozen %d", dtype, relu_mode, frozen);
    return E_INVALID;
  }
  const int V = vec_w(dtype);
  if (M < 1 || C < 1 || C % V || !ld_ok(lddy, C, V)) {
    set_error("fscnn_bn_bwd: M=%lld C=%d lddy=%d (C and lddy a multiple of %d, lddy >= C)", M, C,
              lddy, V);
    return E_INVALID;
  }
  if ((relu_mode == 1) != (mask != nullptr) || (mask && !ld_ok(ldmask, C, V)) ||
      (relu_mode == 2 && !shift)) {
    set_error("fscnn_bn_bwd: relu_mode %d needs %s (ldmask=%d)", relu_mode,
              relu_mode == 1 ? "a mask tensor" : relu_mode == 2 ? "the forward shift and no mask"
                                                                : "no mask", ldmask);
    return E_INVALID;
  }
  const bool pair = z2 != nullptr;
  if (pair && (relu_mode != 1 || frozen == 2 || !mean2 || !invstd2 || !scale2 || !dz2 ||
               !dgamma2 || !dbeta2 || 4 * C > 2048)) {
    set_error("fscnn_bn_bwd: a paired BN needs the mask mode (relu_mode 1), its own statistics, "
              "dz2 / dgamma2 / dbeta2, coefficients passed to the apply and C <= 512");
    return E_INVALID;
  }
  hipStream_t st = S(stream);
  int rpb;
  const int P = bn_bwd_parts(M, C, dtype, &rpb);
  if (P_out) *P_out = P;
  if (rows_per_block_out) *rows_per_block_out = rpb;
  const double count = frozen ? BN_FROZEN_COUNT : (double)M;
  // net.cpp Exec::bn_bwd_stats + bn_bwd, or bn_bwd_pair: reduce, finish(es), apply
  BnBwdArgs b{};
  b.M = M; b.C = C;
  b.dy = dy; b.lddy = lddy; b.mask = mask; b.ldmask = ldmask;
  b.z = z; b.ldz = C;
  b.mean = mean; b.invstd = invstd; b.scale = scale; b.shift = shift;
  b.relu_z = relu_mode == 2;
  b.part = part;
  float* coef2 = coef + 2 * C;
  if (pair) {
    b.z2 = z2; b.mean2 = mean2; b.invstd2 = invstd2; b.scale2 = scale2;
    b.part2 = part + (size_t)P * 2 * C;
  }
  int rc = bn_bwd_reduce(b, dtype, st);
  if (rc) return rc;
  rc = bn_bwd_finalize(b.part, P, C, count, dgamma, dbeta, coef, st, counters, BnBwdTab());
  if (rc) return rc;
  if (pair) {
    rc = bn_bwd_finalize(b.part2, P, C, count, dgamma2, dbeta2, coef2, st, counters, BnBwdTab());
    if (rc) return rc;
    b.coef2 = coef2; b.dz2 = dz2;
  }
  b.coef = frozen == 2 ? nullptr : coef;
  b.dz = dz; b.lddz = C;
  return bn_bwd_apply(b, dtype, st);
}

int fscnn_ppm_branches_ok(int maxM, int K, int dtype) {
  return ppm_branches_ok(maxM, K, dtype) ? 1 : 0;
}

// the branch layout of both PPM calls: rows packed branch after branch (the executor's bin-major
// pooled tensor), per-branch tables [nb][32]
static int ppm_rows(const char* who, int nb, const int* M, int K, int dtype, int off[5]) {
  if (nb < 1 || nb > 4 || !M) {
    set_error("%s: nb=%d (1 .. 4 branches, row counts in M)", who, nb);
    return E_INVALID;
  }
  if (!dt_ok(dtype)) {
    set_error("%s: dtype %d", who, dtype);
    return E_INVALID;
  }
  int maxM = 0;
  off[0] = 0;
  for (int i = 0; i < nb; ++i) {
    if (M[i] < 1) {
      set_error("%s: branch %d has M=%d rows", who, i, M[i]);
      return E_INVALID;
    }
    maxM = std::max(maxM, M[i]);
    off[i + 1] = off[i] + M[i];
  }
  if (!ppm_branches_ok(maxM, K, dtype)) {
    set_error("%s: M=%d K=%d dtype=%d not supported (M <= 512, K a multiple of 8)", who, maxM, K,
              dtype);
    return E_UNSUPPORTED;
  }
  return OK;
}

int fscnn_ppm_branches_fwd(int nb, const int* M, int K, const void* x, const void* w,
                           const float* gamma, const float* beta, float* rmean, float* rvar,
                           long long* nbt, float momentum, void* z, void* y, int ldy, float* mean,
                           float* invstd, float* scale, float* shift, int dtype, void* stream) {
  if (!x || !w || !gamma || !beta || !rmean || !rvar || !z || !y || !mean || !invstd || !scale ||
      !shift) {
    set_error("fscnn_ppm_branches_fwd: null argument");
    return E_INVALID;
  }
  int off[5];
  const int rc = ppm_rows("fscnn_ppm_branches_fwd", nb, M, K, dtype, off);
  if (rc) return rc;
  if (ldy < 32) {
    set_error("fscnn_ppm_branches_fwd: ldy=%d < 32", ldy);
    return E_INVALID;
  }
  const size_t E = dtype == DT_F32 ? 4 : 2;
  // net.cpp forward, "global_feature_extractor.ppm.conv1-4" (fin_args per branch)
  PpmFwdArgs f{};
  f.nb = nb; f.K = K; f.C = 32;
  for (int i = 0; i < nb; ++i) {
    PpmBranchFwd& b = f.b[i];
    b.f.gamma = gamma + 32 * i; b.f.beta = beta + 32 * i;
    b.f.rmean = rmean + 32 * i; b.f.rvar = rvar + 32 * i;
    b.f.nbt = nbt ? nbt + i : nullptr;
    b.f.momentum = momentum;
    b.f.mean = mean + 32 * i; b.f.invstd = invstd + 32 * i;
    b.f.scale = scale + 32 * i; b.f.shift = shift + 32 * i;
    b.f.C = 32;
    b.x = (const char*)x + (size_t)off[i] * K * E;
    b.w = (const char*)w + (size_t)i * 32 * K * E;
    b.z = (char*)z + (size_t)off[i] * 32 * E;
    b.y = (char*)y + (size_t)off[i] * ldy * E;
    b.ldy = ldy; b.M = M[i];
  }
  return ppm_branches_fwd(f, dtype, S(stream));
}

int fscnn_ppm_branches_bwd(int nb, const int* M, int K, const void* dy, int lddy, const void* y,
                           int ldy, const void* z, const float* mean, const float* invstd,
                           const float* scale, const float* gamma, const void* x, const void* w,
                           float* dgamma, float* dbeta, float* dw, void* dx, int dtype,
                           void* stream) {
  if (!dy || !y || !z || !mean || !invstd || !scale || !gamma || !x || !w || !dgamma || !dbeta ||
      !dw || !dx) {
    set_error("fscnn_ppm_branches_bwd: null argument");
    return E_INVALID;
  }
  int off[5];
  const int rc = ppm_rows("fscnn_ppm_branches_bwd", nb, M, K, dtype, off);
  if (rc) return rc;
  if (lddy < 32 || ldy < 32) {
    set_error("fscnn_ppm_branches_bwd: lddy=%d ldy=%d < 32", lddy, ldy);
    return E_INVALID;
  }
  const size_t E = dtype == DT_F32 ? 4 : 2;
  // net.cpp backward_head, "global_feature_extractor.ppm.conv1-4 (backward)"
  PpmBwdArgs f{};
  f.nb = nb; f.K = K; f.C = 32;
  for (int i = 0; i < nb; ++i) {
    PpmBranchBwd& b = f.b[i];
    b.dy = (const char*)dy + (size_t)off[i] * lddy * E; b.lddy = lddy;
    b.y = (const char*)y + (size_t)off[i] * ldy * E; b.ldy = ldy;
    b.z = (const char*)z + (size_t)off[i] * 32 * E;
    b.mean = mean + 32 * i; b.invstd = invstd + 32 * i; b.scale = scale + 32 * i;
    b.gamma = gamma + 32 * i;
    b.x = (const char*)x + (size_t)off[i] * K * E;
    b.w = (const char*)w + (size_t)i * 32 * K * E;
    b.dgamma = dgamma + 32 * i; b.dbeta = dbeta + 32 * i;
    b.dw = dw + (size_t)i * 32 * K;
    b.dx = (char*)dx + (size_t)off[i] * K * E;
    b.M = M[i];
  }
  return ppm_branches_bwd(f, dtype, S(stream));
}

// the concat slice of both PPM upsample calls: 4 levels x 32 channels at channel offset coff
static int ppm_up_check(const char* who, int dtype, int N, int H, int W, int ldy, int coff) {
  if (!dt_ok(dtype)) {
    set_error("%s: dtype %d", who, dtype);
    return E_INVALID;
  }
  const int V = vec_w(dtype);
  if (N < 1 || H < 1 || W < 1 || coff < 0 || coff % V || ldy % V || ldy < coff + 128) {
    set_error("%s: N=%d H=%d W=%d ldy=%d coff=%d (128 channels at coff within ldy, both a "
              "multiple of %d)", who, N, H, W, ldy, coff, V);
    return E_INVALID;
  }
  return OK;
}

int fscnn_ppm_up_fwd(const void* feats, int dtype, int N, int H, int W, void* y, int ldy, int coff,
                     void* stream) {
  if (!feats || !y) {
    set_error("fscnn_ppm_up_fwd: null argument");
    return E_INVALID;
  }
  const int rc = ppm_up_check("fscnn_ppm_up_fwd", dtype, N, H, W, ldy, coff);
  if (rc) return rc;
  PpmUpArgs u{};
  u.N = N; u.H = H; u.W = W; u.CF = 32; u.feats = feats;
  u.y = y; u.ldy = ldy; u.coff = coff;
  return ppm_up_fwd(u, dtype, S(stream));
}

int fscnn_ppm_up_bwd(const void* dy, int dtype, int N, int H, int W, int ldy, int coff,
                     void* dfeats, void* stream) {
  if (!dy || !dfeats) {
    set_error("fscnn_ppm_up_bwd: null argument");
    return E_INVALID;
  }
  const int rc = ppm_up_check("fscnn_ppm_up_bwd", dtype, N, H, W, ldy, coff);
  if (rc) return rc;
  if (H > 80 || N > 65535) {
    set_error("fscnn_ppm_up_bwd: H=%d N=%d (H <= 80: the row sums of a level stay in LDS)", H, N);
    return E_UNSUPPORTED;
  }
  PpmUpArgs u{};
  u.N = N; u.H = H; u.W = W; u.CF = 32; u.feats = nullptr;
  u.y = const_cast<void*>(dy); u.ldy = ldy; u.coff = coff;
  return ppm_up_bwd(u, dfeats, dtype, S(stream));
}

int fscnn_dropout(const void* x, int ldx, int dtype, int N, int H, int W, int C,
                  unsigned long long seed, const unsigned long long* seed_slot,
                  unsigned long long seed_add, float p, const float* x_scale,
                  const float* x_shift, void* y, int ldy, void* stream) {
  if (!x || !y || ((x_scale != nullptr) != (x_shift != nullptr))) {
    set_error("fscnn_dropout: null argument (x_scale and x_shift come together)");
    return E_INVALID;
  }
  if (!dt_ok(dtype) || !(p >= 0.f && p < 1.f)) {
    set_error("fscnn_dropout: dtype %d / p %g", dtype, (double)p);
    return E_INVALID;
  }
  const int V = vec_w(dtype);
  if (N < 1 || H < 1 || W < 1 || C < 1 || C % V || !ld_ok(ldx, C, V) || !ld_ok(ldy, C, V) ||
      (long long)N * H * W * (C / V) >= (1LL << 31)) {
    set_error("fscnn_dropout: N=%d H=%d W=%d C=%d ldx=%d ldy=%d (C, ldx and ldy a multiple of "
              "%d, strides >= C)", N, H, W, C, ldx, ldy, V);
    return E_INVALID;
  }
  // net.cpp forward (classifier Dropout, lazy BN form) / backward_head / forward_aux (seed_add 1)
  DropArgs d{};
  d.N = N; d.H = H; d.W = W; d.C = C; d.x = x; d.ldx = ldx;
  d.x_scale = x_scale; d.x_shift = x_shift;
  d.y = y; d.ldy = ldy; d.seed = seed; d.p = p; d.seed_add = seed_add;
  d.seed_ptr = reinterpret_cast<const uint64_t*>(seed_slot);
  return dropout(d, dtype, S(stream));
}

// geometry shared by the depthwise train wrappers
static int dw_train_check(const char* who, int dtype, int N, int H, int W, int C, int stride) {
  if (!dt_ok(dtype)) {
    set_error("%s: dtype %d", who, dtype);
    return E_INVALID;
  }
  const int V = vec_w(dtype);
  if (N < 1 || H < 1 || W < 1 || C < 1 || C % V || (stride != 1 && stride != 2)) {
    set_error("%s: N=%d H=%d W=%d C=%d stride=%d (C a multiple of %d, stride 1 or 2)", who, N, H,
              W, C, stride, V);
    return E_INVALID;
  }
  return OK;
}

int fscnn_dw3x3_parts(int N, int H, int W, int C, int stride, int dtype, int dgrad) {
  if (dw_train_check("fscnn_dw3x3_parts", dtype, N, H, W, C, stride)) return -1;
  if (dgrad) return dw_dgrad_parts(N, H, W, C, dtype, stride);
  return dw_parts(N, (H - 1) / stride + 1, (W - 1) / stride + 1, C, dtype, stride);
}

int fscnn_dw3x3_ct_width(int N, int H, int W, int C, int stride, int dtype) {
  if (dw_train_check("fscnn_dw3x3_ct_width", dtype, N, H, W, C, stride)) return -1;
  return dw_ct_width(N, (H - 1) / stride + 1, (W - 1) / stride + 1, W, C, dtype, stride);
}

int fscnn_dw3x3_fwd_train(const void* x, int dtype, int N, int H, int W, int C, int stride,
                          const float* w, const float* in_scale, const float* in_shift, void* z,
                          float* part, unsigned* counters, double* tsum, const float* gamma,
                          const float* beta, float* rmean, float* rvar, long long* nbt,
                          float momentum, float* mean, float* invstd, float* scale, float* shift,
                          int* in_kernel, void* stream) {
  if (!x || !w || !z || !part || !counters || !tsum || !gamma || !beta || !rmean || !rvar ||
      !mean || !invstd || !scale || !shift || ((in_scale != nullptr) != (in_shift != nullptr))) {
    set_error("fscnn_dw3x3_fwd_train: null argument (in_scale and in_shift come together)");
    return E_INVALID;
  }
  const int rc = dw_train_check("fscnn_dw3x3_fwd_train", dtype, N, H, W, C, stride);
  if (rc) return rc;
  // net.cpp Exec::dw, train form (fin_args)
  DwArgs d{};
  d.N = N; d.H = H; d.W = W; d.C = C; d.stride = stride;
  d.Ho = (H - 1) / stride + 1; d.Wo = (W - 1) / stride + 1;
  d.x = x; d.w = w; d.in_scale = in_scale; d.in_shift = in_shift;
  d.relu = 0; d.y = z;
  d.part = part;
  d.tail.counters = counters;
  d.tail.tsum = tsum;
  BnFinalizeArgs& f = d.tail.fwd;
  f.part = part; f.C = C;
  f.P = dw_parts(N, d.Ho, d.Wo, C, dtype, stride);
  f.gamma = gamma; f.beta = beta; f.rmean = rmean; f.rvar = rvar; f.nbt = nbt;
  f.momentum = momentum;
  f.mean = mean; f.invstd = invstd; f.scale = scale; f.shift = shift;
  f.counters = counters;
  int P;
  if (in_kernel) *in_kernel = dw_fwd_tail_ink(d, dtype, &P);
  return dw_fwd(d, dtype, S(stream));
}

int fscnn_dw3x3_dgrad_bn(const void* dy, int dtype, int N, int H, int W, int C, int stride,
                         const float* w, void* dx, const void* z, const float* mean,
                         const float* invstd, const float* scale, const float* shift,
                         int relu_mode, float* part, unsigned* counters, double* tsum,
                         float* dgamma, float* dbeta, float* coef, int* in_kernel, void* stream) {
  if (!dy || !w || !dx || !z || !mean || !invstd || !part || !counters || !tsum || !dgamma ||
      !dbeta || !coef) {
    set_error("fscnn_dw3x3_dgrad_bn: null argument");
    return E_INVALID;
  }
  const int rc = dw_train_check("fscnn_dw3x3_dgrad_bn", dtype, N, H, W, C, stride);
  if (rc) return rc;
  if ((relu_mode != 0 && relu_mode != 2) || (relu_mode == 2 && (!scale || !shift))) {
    set_error("fscnn_dw3x3_dgrad_bn: relu_mode %d (0, or 2 with the forward scale and shift)",
              relu_mode);
    return E_INVALID;
  }
  // net.cpp Exec::dw_bwd with a BN target (bt)
  DwBwdArgs d{};
  d.N = N; d.H = H; d.W = W; d.C = C; d.stride = stride;
  d.Ho = (H - 1) / stride + 1; d.Wo = (W - 1) / stride + 1;
  d.dy = dy; d.w = w; d.dx = dx;
  d.bs.part = part; d.bs.z = z;
  d.bs.mean = mean; d.bs.invstd = invstd; d.bs.scale = scale; d.bs.shift = shift;
  d.bs.mode = relu_mode;
  d.tail.counters = counters;
  d.tail.tsum = tsum;
  d.tail.count = (double)N * H * W;
  d.tail.dgamma = dgamma; d.tail.dbeta = dbeta; d.tail.coef = coef;
  int P;
  if (in_kernel) *in_kernel = dw_dgrad_tail_ink(d, dtype, &P);
  return dw_dgrad(d, dtype, S(stream));
}

int fscnn_dw3x3_wgrad_train(const void* x, const void* dy, int dtype, int N, int H, int W, int C,
                            int stride, const float* x_scale, const float* x_shift, float* slab,
                            float* dw, void* stream) {
  if (!x || !dy || !slab || !dw || ((x_scale != nullptr) != (x_shift != nullptr))) {
    set_error("fscnn_dw3x3_wgrad_train: null argument (x_scale and x_shift come together)");
    return E_INVALID;
  }
  int rc = dw_train_check("fscnn_dw3x3_wgrad_train", dtype, N, H, W, C, stride);
  if (rc) return rc;
  // net.cpp Exec::dw_bwd, the weight-gradient half (X = act(u): x_scale / x_shift of a lazy input)
  DwBwdArgs d{};
  d.N = N; d.H = H; d.W = W; d.C = C; d.stride = stride;
  d.Ho = (H - 1) / stride + 1; d.Wo = (W - 1) / stride + 1;
  d.x = x; d.x_scale = x_scale; d.x_shift = x_shift; d.dy = dy; d.slab = slab;
  rc = dw_wgrad(d, dtype, S(stream));
  if (rc) return rc;
  return dw_wgrad_reduce(slab, dw_wgrad_parts(N, d.Ho, d.Wo, C, dtype, stride), C, dw, S(stream));
}

// ---- the pointwise (1x1) train GEMM forms and the aux head's column kernels, in the executor's
// form (tests/test_gpu_train_gemm.py)
static int pw_geom_check(const char* who, int dtype, int M, int N, int K, int lda, int ldb,
                         int ldc) {
  if (!dt_ok(dtype)) {
    set_error("%s: dtype %d", who, dtype);
    return E_INVALID;
  }
  const int V = vec_w(dtype);
  if (M < 1 || N < 1 || K < 1 || !ld_ok(lda, K, V) || !ld_ok(ldb, K, V) || ldc < N) {
    set_error("%s: M=%d N=%d K=%d, row strides %d / %d / %d (the operands' >= K and a multiple "
              "of %d, the output's >= N)", who, M, N, K, lda, ldb, ldc, V);
    return E_INVALID;
  }
  return OK;
}
// 0: the streaming kernel (its last workgroup finishes the BN), 1: the tiled kernel finishing the
// BN in its last workgroups, 2: the tiled kernel followed by the finalize launch
static int pw_route(const GemmArgs& g, int dtype, int* records) {
  int P;
  const int ink = gemm_nt_tail_ink(g, dtype, &P);
  if (records) *records = P;
  return gemm_stream_ok(g, dtype) ? 0 : (ink ? 1 : 2);
}

// net.cpp Exec::pw (train branch) + gemm_fin + fin_args, field for field
static GemmArgs pw_fwd_train_args(int M, int N, int K, const void* A, int lda,
                                  const float* a_scale, const float* a_shift, const void* B,
                                  int ldb, const float* bias, void* z, int ldc, float* part,
                                  unsigned* counters, double* tsum, const BnFinalizeArgs& bn) {
  GemmArgs g{};
  g.M = M; g.N = N; g.K = K;
  g.A = A; g.lda = lda; g.a_scale = a_scale; g.a_shift = a_shift;   // In x (act(u): lazy)
  g.B = B; g.ldb = ldb; g.b_trans = 0;                              // Wg(c), ldb = K
  g.scale = nullptr; g.shift = bias;                                // P(c.b)
  g.C = z; g.ldc = ldc;                                             // W(u.z), u.C
  g.part = part;                                                    // gemm_fin: Wf(u.part)
  g.tail.counters = counters;                                       // pl.fcnt
  g.tail.fwd = bn;                                                  // fin_args(u)
  g.tail.fwd.part = part; g.tail.fwd.C = N;
  g.tail.fwd.bias = nullptr;
  g.tail.fwd.counters = counters;
  g.tail.tsum = tsum;                                               // pl.tsum
  return g;
}

static int pw_fwd_train_check(int M, int N, int K, int lda, int ldb, int ldc, int lazy, int dtype) {
  const int rc = pw_geom_check("fscnn_pw_fwd_train", dtype, M, N, K, lda, ldb, ldc);
  if (rc) return rc;
  if (N > 1024 || (lazy && (K % vec_w(dtype) || K > 768))) {
    set_error("fscnn_pw_fwd_train: N=%d K=%d (N <= 1024; a lazy operand needs K <= 768 and a "
              "multiple of %d)", N, K, vec_w(dtype));
    return E_INVALID;
  }
  return OK;
}

int fscnn_pw_fwd_train_route(int M, int N, int K, int lda, int ldc, int lazy, int dtype,
                             int* records) {
  if (pw_fwd_train_check(M, N, K, lda, lda, ldc, lazy, dtype)) return -1;  // (B's stride: no part)
  static float f;     // host-side planning only reads which pointers are set
  static unsigned u;
  static double d;
  const GemmArgs g = pw_fwd_train_args(M, N, K, &f, lda, lazy ? &f : nullptr, lazy ? &f : nullptr,
                                       &f, lda, nullptr, &f, ldc, &f, &u, &d, BnFinalizeArgs{});
  return pw_route(g, dtype, records);
}

int fscnn_pw_fwd_train(int M, int N, int K, const void* A, int lda, const float* a_scale,
                       const float* a_shift, const void* B, int ldb, const float* bias, void* z,
                       int ldc, float* part, unsigned* counters, double* tsum, const float* gamma,
                       const float* beta, float* rmean, float* rvar, long long* nbt,
                       float momentum, float* mean, float* invstd, float* scale, float* shift,
                       int dtype, int* route, int* records, void* stream) {
  if (!A || !B || !z || !part || !counters || !tsum || !gamma || !beta || !rmean || !rvar ||
      !mean || !invstd || !scale || !shift || ((a_scale != nullptr) != (a_shift != nullptr))) {
    set_error("fscnn_pw_fwd_train: null argument (a_scale and a_shift come together)");
    return E_INVALID;
  }
  const int rc = pw_fwd_train_check(M, N, K, lda, ldb, ldc, a_scale != nullptr, dtype);
  if (rc) return rc;
  BnFinalizeArgs f{};  // fin_args(u); P is set by the finish that runs
  f.gamma = gamma; f.beta = beta; f.rmean = rmean; f.rvar = rvar; f.nbt = nbt;
  f.momentum = momentum;
  f.mean = mean; f.invstd = invstd; f.scale = scale; f.shift = shift;
  const GemmArgs g = pw_fwd_train_args(M, N, K, A, lda, a_scale, a_shift, B, ldb, bias, z, ldc,
                                       part, counters, tsum, f);
  int P;
  const int rt = pw_route(g, dtype, &P);
  if (route) *route = rt;
  if (records) *records = P;
  return gemm_nt(g, dtype, S(stream));
}

int fscnn_pw_wgrad_train(int M, int N, int K, const void* D, int ldd, const void* X, int ldx,
                         const float* x_scale, const float* x_shift, float* slab, float* dW,
                         float* bias_part, float* dbias, int dtype, int* splits, void* stream) {
  if (!D || !X || !slab || !dW || ((x_scale != nullptr) != (x_shift != nullptr)) ||
      ((bias_part != nullptr) != (dbias != nullptr))) {
    set_error("fscnn_pw_wgrad_train: null argument (x_scale / x_shift and bias_part / dbias come "
              "together)");
    return E_INVALID;
  }
  if (!dt_ok(dtype)) {
    set_error("fscnn_pw_wgrad_train: dtype %d", dtype);
    return E_INVALID;
  }
  const int V = vec_w(dtype);
  if (M < 1 || N < 1 || K < 1 || !ld_ok(ldd, N, V) || !ld_ok(ldx, K, V) || (x_scale && K % V)) {
    set_error("fscnn_pw_wgrad_train: M=%d N=%d K=%d ldd=%d ldx=%d (ldd >= N, ldx >= K, both a "
              "multiple of %d; a lazy X needs K a multiple of it too)", M, N, K, ldd, ldx, V);
    return E_INVALID;
  }
  hipStream_t st = S(stream);
  // net.cpp Exec::pw_bwd, the weight-gradient half: gemm_tn + reduce (+ colsum + reduce: c.b)
  GemmTnArgs t{};
  t.M = M; t.N = N; t.K = K; t.D = D; t.ldd = ldd; t.X = X; t.ldx = ldx;  // dz, In X
  t.x_scale = x_scale; t.x_shift = x_shift;                               // X.sc, X.sh
  const int s = gemm_tn_splits(M, N, K);
  t.slab = slab;
  if (splits) *splits = s;
  int rc = gemm_tn(t, s, dtype, st);
  if (rc) return rc;
  rc = reduce_slabs(slab, s, (long long)N * K, (long long)N * K, dW, 0, st);
  if (rc || !dbias) return rc;
  rc = colsum(D, M, N, ldd, bias_part, dtype, st);
  if (rc) return rc;
  return reduce_slabs(bias_part, colsum_parts(M), N, N, dbias, 0, st);
}

// net.cpp Exec::pw_dgrad_args + set_btarget + bwd_tab, field for field
static GemmArgs pw_dgrad_train_args(int M, int N, int K, const void* D, int ldd, const void* B,
                                    int ldb, const void* R, int ldr, void* dX, int lddx,
                                    const void* z, int ldz, const float* mean, const float* invstd,
                                    const float* scale, const float* shift, int relu_mode,
                                    float* part, unsigned* counters, double* tsum, float* dgamma,
                                    float* dbeta, float* coef, float* tab, int drop_hw,
                                    float drop_p, unsigned long long seed,
                                    unsigned long long seed_add,
                                    const unsigned long long* seed_slot) {
  GemmArgs g{};
  g.M = M; g.N = N; g.K = K; g.A = D; g.lda = ldd;           // dz
  g.B = B; g.ldb = ldb; g.b_trans = 0;                       // WT(c), c.ldt
  g.R = R; g.ldr = ldr;
  g.C = dX; g.ldc = lddx;
  g.bpart = part;                                            // pl.bnpart
  g.bz = z; g.ldbz = ldz;                                    // W(u.z), u.C
  g.bmean = mean; g.binvstd = invstd; g.bscale = scale; g.bshift = shift;
  g.bmode = relu_mode;
  g.tail.counters = counters;                                // pl.bcnt
  g.tail.tsum = tsum;
  g.tail.count = (double)M;                                  // bcount(u)
  g.tail.dgamma = dgamma; g.tail.dbeta = dbeta; g.tail.coef = coef;
  g.tail.tab.tab = tab;                                      // bwd_tab(u, mode == 2, slot)
  g.tail.tab.scale = scale; g.tail.tab.shift = shift; g.tail.tab.mean = mean;
  g.tail.tab.invstd = invstd;
  g.tail.tab.relu = relu_mode == 2;
  if (drop_hw > 0) {                                         // dro
    g.drop_hw = drop_hw; g.drop_thr = dropout_threshold(drop_p); g.drop_p = drop_p;
    g.drop_seed = seed; g.drop_seed_ptr = reinterpret_cast<const uint64_t*>(seed_slot);
    g.drop_seed_add = seed_add;
  }
  return g;
}

static int pw_dgrad_train_check(int M, int N, int K, int ldd, int ldb, int ldr, int has_r,
                                int lddx, int ldz, int relu_mode, int drop_hw, float drop_p,
                                int dtype) {
  const int rc = pw_geom_check("fscnn_pw_dgrad_train", dtype, M, N, K, ldd, ldb, lddx);
  if (rc) return rc;
  const int V = vec_w(dtype);
  if ((relu_mode != 0 && relu_mode != 2) || N > 1024 || !ld_ok(ldz, N, V) ||
      (has_r && !ld_ok(ldr, N, V))) {
    set_error("fscnn_pw_dgrad_train: relu_mode %d N=%d ldz=%d ldr=%d (relu_mode 0 or 2, N <= 1024, "
              "ldz / ldr >= N and a multiple of %d)", relu_mode, N, ldz, ldr, V);
    return E_INVALID;
  }
  if (drop_hw < 0 || (drop_hw > 0 && (!(drop_p >= 0.f && drop_p < 1.f) || M % drop_hw))) {
    set_error("fscnn_pw_dgrad_train: dropout hw %d p %g (0 <= p < 1, M a multiple of hw)", drop_hw,
              (double)drop_p);
    return E_INVALID;
  }
  return OK;
}

static int pw_dgrad_drop_check(const GemmArgs& g, int dtype) {
  if (g.drop_hw && !gemm_stream_ok(g, dtype)) {
    set_error("fscnn_pw_dgrad_train: an output dropout needs the streaming kernel, which does "
              "not take M=%d N=%d K=%d in dtype %d", g.M, g.N, g.K, dtype);
    return E_UNSUPPORTED;
  }
  return OK;
}

int fscnn_pw_dgrad_train_route(int M, int N, int K, int ldd, int lddx, int residual, int drop_hw,
                               int dtype, int* records) {
  if (pw_dgrad_train_check(M, N, K, ldd, ldd, lddx, residual, lddx, lddx, 0, drop_hw, 0.1f, dtype))
    return -1;
  static float f;     // host-side planning only reads which pointers are set
  static unsigned u;
  static double d;
  const GemmArgs g = pw_dgrad_train_args(M, N, K, &f, ldd, &f, ldd, residual ? &f : nullptr, lddx,
                                         &f, lddx, &f, lddx, &f, &f, &f, &f, 0, &f, &u, &d, &f,
                                         &f, &f, &f, drop_hw, 0.1f, 0, 0, nullptr);
  if (pw_dgrad_drop_check(g, dtype)) return -1;
  return pw_route(g, dtype, records);
}

int fscnn_pw_dgrad_train(int M, int N, int K, const void* D, int ldd, const void* B, int ldb,
                         const void* R, int ldr, void* dX, int lddx, const void* z, int ldz,
                         const float* mean, const float* invstd, const float* scale,
                         const float* shift, int relu_mode, float* part, unsigned* counters,
                         double* tsum, float* dgamma, float* dbeta, float* coef, float* tab,
                         int drop_hw, float drop_p, unsigned long long seed,
                         unsigned long long seed_add, const unsigned long long* seed_slot,
                         int dtype, int* route, int* records, void* stream) {
  if (!D || !B || !dX || !z || !mean || !invstd || !scale || !shift || !part || !counters ||
      !tsum || !dgamma || !dbeta || !coef || !tab || (uintptr_t)tab % 16) {
    set_error("fscnn_pw_dgrad_train: null argument (or tab not 16-byte aligned)");
    return E_INVALID;
  }
  int rc = pw_dgrad_train_check(M, N, K, ldd, ldb, ldr, R != nullptr, lddx, ldz, relu_mode,
                                drop_hw, drop_p, dtype);
  if (rc) return rc;
  const GemmArgs g = pw_dgrad_train_args(M, N, K, D, ldd, B, ldb, R, ldr, dX, lddx, z, ldz, mean,
                                         invstd, scale, shift, relu_mode, part, counters, tsum,
                                         dgamma, dbeta, coef, tab, drop_hw, drop_p, seed, seed_add,
                                         seed_slot);
  rc = pw_dgrad_drop_check(g, dtype);
  if (rc) return rc;
  int P;
  const int rt = pw_route(g, dtype, &P);
  if (route) *route = rt;
  if (records) *records = P;
  return gemm_nt(g, dtype, S(stream));
}

// geometry shared by the aux head's column kernels
static int col3_check(const char* who, int dtype, int N, int H, int W, int C, const void* x, int ldx,
                      const void* col, int ldcol) {
  if (!x || !col) {
    set_error("%s: null argument", who);
    return E_INVALID;
  }
  if (!dt_ok(dtype)) {
    set_error("%s: dtype %d", who, dtype);
    return E_INVALID;
  }
  if (N < 1 || H < 1 || W < 1 || C < 1 || ldx < C || ldcol < 9 * C) {
    set_error("%s: N=%d H=%d W=%d C=%d, row strides %d (>= C) and %d (>= 9 C)", who, N, H, W, C,
              ldx, ldcol);
    return E_INVALID;
  }
  return OK;
}

int fscnn_im2col3(const void* x, int ldx, int dtype, int N, int H, int W, int C, void* col,
                  int ldcol, void* stream) {
  const int rc = col3_check("fscnn_im2col3", dtype, N, H, W, C, x, ldx, col, ldcol);
  if (rc) return rc;
  // net.cpp Exec::forward_aux
  Im2ColArgs a{};
  a.N = N; a.H = H; a.W = W; a.C = C; a.x = x; a.ldx = ldx; a.col = col; a.ldcol = ldcol;
  return im2col3(a, dtype, S(stream));
}

int fscnn_col2im3(const void* dcol, int ldcol, int dtype, int N, int H, int W, int C, void* dx,
                  int lddx, int accumulate, void* stream) {
  const int rc = col3_check("fscnn_col2im3", dtype, N, H, W, C, dx, lddx, dcol, ldcol);
  if (rc) return rc;
  // net.cpp Exec::backward_aux (accumulate = 1 there)
  Col2ImArgs a{};
  a.N = N; a.H = H; a.W = W; a.C = C; a.dcol = dcol; a.ldcol = ldcol; a.dx = dx; a.lddx = lddx;
  a.accumulate = accumulate != 0;
  return col2im3(a, dtype, S(stream));
}

int fscnn_block_ir_fwd(const void* x, int ldx, int dtype, int N, int H, int W, int cin, int expand,
                       int cout, const void* w_expand, const float* w_dw, const void* w_project,
                       const float* scale_e, const float* shift_e, const float* scale_d,
                       const float* shift_d, const float* scale_p, const float* shift_p,
                       int residual, void* y, int ldy, void* stream) {
  if (!x || !y || !w_expand || !w_dw || !w_project || !scale_e || !shift_e || !scale_d ||
      !shift_d || !scale_p || !shift_p) {
    set_error("fscnn_block_ir_fwd: null argument");
    return E_INVALID;
  }
  if (dtype < DT_F32 || dtype > DT_F16) {
    set_error("fscnn_block_ir_fwd: dtype %d", dtype);
    return E_INVALID;
  }
  IrArgs a{};
  a.N = N; a.H = H; a.W = W; a.Cin = cin; a.E = expand; a.Cout = cout;
  a.x = x; a.ldx = ldx; a.y = y; a.ldy = ldy;
  a.we = w_expand; a.wd = w_dw; a.wp = w_project;
  a.sc_e = scale_e; a.sh_e = shift_e; a.sc_d = scale_d; a.sh_d = shift_d;
  a.sc_p = scale_p; a.sh_p = shift_p; a.residual = residual;
  return ir_block_fwd(a, dtype, S(stream));
}

int fscnn_block_ir_s2_fwd(const void* x, int ldx, int dtype, int N, int H, int W, int cin,
                          int expand, int cout, const void* w_expand, const float* w_dw,
                          const void* w_project, const float* scale_e, const float* shift_e,
                          const float* scale_d, const float* shift_d, const float* scale_p,
                          const float* shift_p, void* y, int ldy, void* stream) {
  if (!x || !y || !w_expand || !w_dw || !w_project || !scale_e || !shift_e || !scale_d ||
      !shift_d || !scale_p || !shift_p) {
    set_error("fscnn_block_ir_s2_fwd: null argument");
    return E_INVALID;
  }
  if (dtype < DT_F32 || dtype > DT_F16 || H < 1 || W < 1) {
    set_error("fscnn_block_ir_s2_fwd: dtype %d H %d W %d", dtype, H, W);
    return E_INVALID;
  }
  IrArgs a{};
  a.stride = 2; a.Hi = H; a.Wi = W;
  a.N = N; a.H = (H - 1) / 2 + 1; a.W = (W - 1) / 2 + 1; a.Cin = cin; a.E = expand; a.Cout = cout;
  a.x = x; a.ldx = ldx; a.y = y; a.ldy = ldy;
  a.we = w_expand; a.wd = w_dw; a.wp = w_project;
  a.sc_e = scale_e; a.sh_e = shift_e; a.sc_d = scale_d; a.sh_d = shift_d;
  a.sc_p = scale_p; a.sh_p = shift_p; a.residual = 0;
  return ir_block_fwd(a, dtype, S(stream));
}

int fscnn_block_ltd_fwd(const void* x, int x_dtype, int dtype, int N, int H, int W,
                        const float* w_conv, const float* scale_0, const float* shift_0,
                        const float* w_dw, const float* scale_d, const float* shift_d,
                        const void* w_pw, const float* scale_p, const float* shift_p, void* y,
                        int ldy, void* stream) {
  if (!x || !y || !w_conv || !scale_0 || !shift_0 || !w_dw || !scale_d || !shift_d || !w_pw ||
      !scale_p || !shift_p) {
    set_error("fscnn_block_ltd_fwd: null argument");
    return E_INVALID;
  }
  if (dtype < DT_F32 || dtype > DT_F16 || x_dtype < 0 || x_dtype > 2 || H < 3 || W < 3) {
    set_error("fscnn_block_ltd_fwd: dtype %d x_dtype %d H %d W %d", dtype, x_dtype, H, W);
    return E_INVALID;
  }
  StemArgs a{};
  a.x = x; a.x_dtype = x_dtype;
  a.N = N; a.H = H; a.W = W;
  a.H1 = (H - 3) / 2 + 1; a.W1 = (W - 3) / 2 + 1;
  a.H2 = (a.H1 - 1) / 2 + 1; a.W2 = (a.W1 - 1) / 2 + 1;
  a.w0 = w_conv; a.sc0 = scale_0; a.sh0 = shift_0;
  a.wd = w_dw; a.scd = scale_d; a.shd = shift_d;
  a.wp = w_pw; a.scp = scale_p; a.shp = shift_p;
  a.y = y; a.ldy = ldy;
  return stem_fwd(a, dtype, S(stream));
}

int fscnn_block_dsconv_fwd(const void* x, int dtype, int N, int H, int W, int C, int Co,
                           const float* w_dw, const float* scale_d, const float* shift_d,
                           const void* w_pw, const float* scale_p, const float* shift_p, void* y,
                           int ldy, void* stream) {
  if (!x || !y || !w_dw || !scale_d || !shift_d || !w_pw || !scale_p || !shift_p) {
    set_error("fscnn_block_dsconv_fwd: null argument");
    return E_INVALID;
  }
  if (dtype < DT_F32 || dtype > DT_F16 || N <= 0 || H <= 0 || W <= 0) {
    set_error("fscnn_block_dsconv_fwd: dtype %d N %d H %d W %d", dtype, N, H, W);
    return E_INVALID;
  }
  DsArgs a{};
  a.x = x; a.N = N; a.H = H; a.W = W; a.C = C; a.Co = Co;
  a.wd = w_dw; a.scd = scale_d; a.shd = shift_d;
  a.wp = w_pw; a.scp = scale_p; a.shp = shift_p;
  a.y = y; a.ldy = ldy;
  a.rs = ds_rows(N, H, W);
  return ds_fwd(a, dtype, S(stream));
}

int fscnn_block_dsconv_res_fwd(const void* x, int dtype, int N, int H, int W, int C, int Co,
                               int Hi, int Wi, const float* w_dw, const float* scale_d, const float* shift_d,
                               const void* w_pw, const float* scale_p, const float* shift_p,
                               const void* res, int ldres, void* y, int ldy, void* stream) {
  if (!x || !y || !res || !w_dw || !scale_d || !shift_d || !w_pw || !scale_p || !shift_p) {
    set_error("fscnn_block_dsconv_res_fwd: null argument");
    return E_INVALID;
  }
  if (dtype < DT_F32 || dtype > DT_F16 || N <= 0 || H <= 0 || W <= 0) {
    set_error("fscnn_block_dsconv_res_fwd: dtype %d N %d H %d W %d", dtype, N, H, W);
    return E_INVALID;
  }
  DsArgs a{};
  a.x = x; a.N = N; a.H = H; a.W = W; a.C = C; a.Co = Co;
  a.wd = w_dw; a.scd = scale_d; a.shd = shift_d;
  a.wp = w_pw; a.scp = scale_p; a.shp = shift_p;
  a.r = res; a.ldr = ldres;
  a.Hi = Hi > 0 ? Hi : 0; a.Wi = Hi > 0 ? Wi : 0;
  a.y = y; a.ldy = ldy;
  a.rs = ds_rows(N, H, W);
  return ds_fwd(a, dtype, S(stream));
}

int fscnn_block_cls_fwd(const void* x, int dtype, int N, int H, int W, const float* w_dw1,
                        const float* scale_d1, const float* shift_d1, const void* w_pw1,
                        const float* scale_p1, const float* shift_p1, const float* w_dw2,
                        const float* scale_d2, const float* shift_d2, const void* w_pw2,
                        const float* scale_p2, const float* shift_p2, const void* w_cls,
                        const float* b_cls, int ncls, void* tmp, void* logits, int ldl,
                        void* stream) {
  if (!x || !tmp || !logits || !w_dw1 || !scale_d1 || !shift_d1 || !w_pw1 || !scale_p1 ||
      !shift_p1 || !w_dw2 || !scale_d2 || !shift_d2 || !w_pw2 || !scale_p2 || !shift_p2 || !w_cls ||
      !b_cls) {
    set_error("fscnn_block_cls_fwd: null argument");
    return E_INVALID;
  }
  if (dtype < DT_F32 || dtype > DT_F16 || N <= 0 || H <= 0 || W <= 0) {
    set_error("fscnn_block_cls_fwd: dtype %d N %d H %d W %d", dtype, N, H, W);
    return E_INVALID;
  }
  DsArgs a{};  // dsconv1 -> tmp
  a.x = x; a.N = N; a.H = H; a.W = W; a.C = 128; a.Co = 128;
  a.wd = w_dw1; a.scd = scale_d1; a.shd = shift_d1;
  a.wp = w_pw1; a.scp = scale_p1; a.shp = shift_p1;
  a.y = tmp; a.ldy = 128;
  a.rs = ds_rows(N, H, W);
  DsArgs b = a;  // dsconv2 + the classifier conv -> logits
  b.x = tmp;
  b.wd = w_dw2; b.scd = scale_d2; b.shd = shift_d2;
  b.wp = w_pw2; b.scp = scale_p2; b.shp = shift_p2;
  b.wc = w_cls; b.bc = b_cls; b.ncls = ncls; b.logits = logits; b.ldl = ldl;
  if (!ds_ok(a) || !ds_ok(b)) {
    set_error("fscnn_block_cls_fwd: unsupported shape N=%d H=%d W=%d ncls=%d ldl=%d", N, H, W, ncls, ldl);
    return E_UNSUPPORTED;
  }
  const int rc = ds_fwd(a, dtype, S(stream));
  return rc ? rc : ds_fwd(b, dtype, S(stream));
}

int fscnn_block_ffm_fwd(const void* low, int dtype, int N, int Hi, int Wi, int H, int W,
                        const void* high, int ldhigh, const float* w_dw, const float* scale_d,
                        const float* shift_d, const void* w_low, const float* scale_l,
                        const float* shift_l, const void* w_high, const float* scale_h,
                        const float* shift_h, void* y, int ldy, void* stream) {
  if (!low || !high || !y || !w_dw || !scale_d || !shift_d || !w_low || !scale_l || !shift_l ||
      !w_high || !scale_h || !shift_h) {
    set_error("fscnn_block_ffm_fwd: null argument");
    return E_INVALID;
  }
  if (dtype < DT_F32 || dtype > DT_F16 || N <= 0 || H <= 0 || W <= 0 || Hi <= 0 || Wi <= 0) {
    set_error("fscnn_block_ffm_fwd: dtype %d N %d Hi %d Wi %d H %d W %d", dtype, N, Hi, Wi, H, W);
    return E_INVALID;
  }
  DsArgs a{};
  a.x = low; a.N = N; a.H = H; a.W = W; a.C = 128; a.Co = 128; a.Hi = Hi; a.Wi = Wi;
  a.wd = w_dw; a.scd = scale_d; a.shd = shift_d;
  a.wp = w_low; a.scp = scale_l; a.shp = shift_l;
  a.xh = high; a.ldxh = ldhigh; a.wh = w_high; a.sch = scale_h; a.shh = shift_h;
  a.y = y; a.ldy = ldy;
  a.rs = ds_rows(N, H, W);
  return ds_fwd(a, dtype, S(stream));
}

}  // extern "C"

extern "C" int fscnn_plan_buffer(const fscnn_plan* plan, const char* name, long long* offset,
                                 long long* rows, int* cols, int* ld, int* in_bws) {
  if (!plan || !name) { set_error("fscnn_plan_buffer: null argument"); return E_INVALID; }
  for (const auto& b : plan->plan.named) {
    if (b.name == name) {
      if (offset) *offset = (long long)b.off;
      if (rows) *rows = b.rows;
      if (cols) *cols = b.cols;
      if (ld) *ld = b.ld;
      if (in_bws) *in_bws = b.bws;
      return OK;
    }
  }
  set_error("fscnn_plan_buffer: no buffer named '%s' in this plan", name);
  return E_INVALID;
}
