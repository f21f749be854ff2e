// Native executor of the Fast-SCNN hot path: layer table (state_dict schema of
// models/fast_scnn.py), workspace planning and the forward / backward launch sequences.
// It never allocates device memory: the caller passes the parameter / buffer / gradient arenas
// and workspaces (see include/fastscnn.h).
#pragma once
#include <atomic>
#include <string>
#include <memory>
#include <vector>

#include "kernels.hpp"

namespace fscnn {

struct TSpec {
  std::string name;
  std::vector<int> shape;
  long long off;    // element offset in its arena
  long long numel;
};

struct ConvL {
  long long w = -1, b = -1;  // offsets into P (floats), -1 = none
  int cin = 0, cout = 0, k = 1, groups = 1;
  // dense convs: W^T [cin*k*k][ldt] (zero-padded to ldt = cout rounded up to 8) in the compute
  // dtype at element offset wt of the plan's transposed-weight arena (the dgrad's B operand)
  long long wt = -1;
  int ldt = 0;
};
struct BnL {
  long long g = -1, b = -1;   // P offsets
  long long rm = -1, rv = -1; // R offsets
  int nbt = -1;               // index into the num_batches_tracked arena
  int C = 0;
  int id = -1;                // BN ordinal
};
struct DsL { ConvL dw; BnL bdw; ConvL pw; BnL bpw; };
struct LbL { ConvL e; BnL be; ConvL d; BnL bd; ConvL p; BnL bp; int cin, cout, stride; };

struct Net {
  int num_classes = 0, aux = 0;
  std::vector<TSpec> params;   // P arena (fp32), named_parameters() order
  std::vector<TSpec> buffers;  // R arena (fp32 running_mean/var) + nbt entries (off = index)
  long long p_total = 0, r_total = 0;
  int n_bn = 0;
  ConvL c0; BnL b0;
  DsL ltd1, ltd2, cls1, cls2;
  LbL lb[9];
  ConvL ppm_c[4]; BnL ppm_b[4];
  ConvL ppm_o; BnL ppm_ob;
  ConvL ffm_dw; BnL ffm_bdw;
  ConvL ffm_low; BnL ffm_blow;
  ConvL ffm_high; BnL ffm_bhigh;
  ConvL cls_out;
  ConvL aux0; BnL aux1; ConvL aux4;
  long long stage_p_begin[4];  // P offset where each backward stage's parameters start
  long long wt_total = 0;      // elements of the transposed-weight arena
};

int net_build(int num_classes, int aux, Net& net);

// the PPM's pooled / branch tensors are bin-major [50][N][C]: bin sizes and first bin per branch
constexpr int PPM_BINS[4] = {1, 2, 3, 6}, PPM_BASE[4] = {0, 1, 5, 14};

enum { U_CONV0 = 0, U_DW = 1, U_PW = 2 };  // Unit::kind

// A conv+BN output in the workspace, and the layer that produces it.
struct Unit {
  int kind = U_PW;          // first conv / depthwise 3x3 / pointwise (GEMM; the aux 3x3 on im2col)
  const ConvL* conv = nullptr;  // into *Plan::net
  const BnL* bn = nullptr;
  int Hi = 0, Wi = 0, Ho = 0, Wo = 0, stride = 0;  // depthwise units: input / output map
  long long M = 0;
  int C = 0, ld = 0;
  size_t z = 0, a = 0;      // raw conv output / activation (same in eval)
  size_t part = 0;          // BN partial records
  int nparts = 0;           // record slots (gemm_parts(M) for GEMM producers: an upper bound)
  // the dgrad producing this unit's dy (GEMM or depthwise) also reduces and finishes its BN
  // backward (set when that dgrad is issued; fixed per plan): the BN backward then only applies
  // (an atomic: concurrent backward calls of DataParallel replicas set it; always to true)
  struct Flag {
    std::atomic<bool> v{false};
    Flag() = default;
    Flag(const Flag& o) : v(o.v.load(std::memory_order_relaxed)) {}
    Flag& operator=(const Flag& o) {
      v.store(o.v.load(std::memory_order_relaxed), std::memory_order_relaxed);
      return *this;
    }
    bool get() const { return v.load(std::memory_order_relaxed); }
    void set() const { const_cast<std::atomic<bool>&>(v).store(true, std::memory_order_relaxed); }
  };
  Flag bdone;
  size_t mean = 0, invstd = 0, scale = 0, shift = 0;  // fp32 [C]
  size_t ga = 0;            // backward: grad wrt a (bwd workspace)
  int ga_ld = 0;
  // train: the BN+ReLU output is never stored; every consumer (forward GEMM / depthwise and the
  // backward wgrads) applies relu(fmaf(z, scale, shift)) to z while staging its operand
  bool lazy = false;
  std::string name;         // reference module path (per-launch profile label)
  std::string key;          // short name of its debug buffers ("lbe3.z", fscnn_plan_buffer)
  std::string block_name;   // label of a fused whole-block launch (inference bottlenecks)
};

struct GraphCache;
struct SideStream;

struct Plan {
  const Net* net = nullptr;
  int N = 0, H = 0, W = 0, dtype = DT_F32, train = 0;
  int H1, W1, H2, W2, H3, W3, H4, W4, H5, W5;
  int Cp = 0;   // padded class count (row stride of the low-res logits)
  size_t ws_bytes = 0, bws_bytes = 0;
  size_t slab_floats = 0;  // weight-gradient partial arena (every job of a step has its own slab)
  // forward units
  Unit c0, l1dw, l1pw, l2dw, l2pw;
  Unit lbe[9], lbd[9], lbp[9];
  Unit ppk[4], po;
  Unit fdw, flow, fhigh;
  Unit c1dw, c1pw, c2dw, c2pw;
  Unit aux0;
  size_t concat = 0, pooled = 0, feats_a = 0, up_low = 0, f = 0, drop = 0,
         logits = 0, aux_drop = 0, aux_logits = 0, aux_col = 0, pbf = 0;
  size_t wt = 0;                    // transposed weights (train plans), net.wt_total elements
  size_t lb_we3[9] = {}, lb_wp3[9] = {};  // fp32 inference: split planes of fused bottlenecks
  size_t g_raw = 0, head_part = 0;  // fused loss head (train plans)
  size_t tgt8 = 0;                    // the loss head's int8 targets (train plans)
  size_t seed_slot = 0;             // dropout seed (device copy read by the dropout kernels)
  size_t fcnt = 0, bcnt = 0;        // BN arrival counters (ws), BN_COUNTERS each
  size_t tsum = 0;                  // fp64 team sums of the in-kernel BN finishes (ws)
  size_t tsum2 = 0;                 // ... of the forward's side-stream producer (FFM high-res)
  // backward workspace
  size_t g_logits = 0, t_up = 0, g_drop = 0, g_f = 0, g_up = 0, t_up2 = 0, g_concat = 0,
         g_feats = 0, g_pooled = 0, dz = 0, slab = 0, bnpart = 0, coef = 0, cspart = 0,
         g_aux = 0, g_auxlog = 0, aux_dcol = 0, xtab = 0, c0sum = 0;
  size_t dz_bytes = 0;             // the dz arena (one slot per unit, Exec::dz_buf)
  size_t bnpart_floats = 0;        // capacity of the BN-backward record arena (bnpart)
  // named buffers for debugging / stage-level parity: name -> (offset, rows, cols, ld, in_bws)
  struct Named { std::string name; size_t off; long long rows; int cols, ld, bws; };
  std::vector<Named> named;
  // captured hipGraphs of whole forward / backward-stage calls, keyed by their arguments
  std::shared_ptr<GraphCache> graphs;
  // second stream for the weight-gradient launches of the backward (created on first use)
  std::shared_ptr<SideStream> side;
};

// Every unit of a plan (Plan& or const Plan&) in forward order; aux0 only for aux nets.  This
// and plan_build's two allocation sequences are the only places that list the units.  (A
// function, not a table of Unit* in the plan: plans are copied.)
template <class P, class F>
void for_each_unit(P& pl, F&& f) {
  f(pl.c0); f(pl.l1dw); f(pl.l1pw); f(pl.l2dw); f(pl.l2pw);
  for (int i = 0; i < 9; ++i) { f(pl.lbe[i]); f(pl.lbd[i]); f(pl.lbp[i]); }
  for (int i = 0; i < 4; ++i) f(pl.ppk[i]);
  f(pl.po); f(pl.fdw); f(pl.flow); f(pl.fhigh);
  f(pl.c1dw); f(pl.c1pw); f(pl.c2dw); f(pl.c2pw);
  if (pl.net->aux) f(pl.aux0);
}

int plan_build(const Net& net, int N, int H, int W, int dtype, int train, Plan& pl);
bool ir_block_shape(const Plan& pl, int i, IrArgs& b);
std::shared_ptr<GraphCache> make_graph_cache();
std::shared_ptr<SideStream> make_side_stream();

enum { HEAD_CE = 0, HEAD_DICE = 1, HEAD_OHEM = 2 };

struct RunArgs {
  const void* x; int x_dtype;     // NCHW input image
  void* out; int out_dtype;       // NCHW logits [N][C][H][W]
  void* aux_out;                  // NCHW aux logits or null
  const float* P;                 // parameter arena
  float* R;                       // running stats arena
  long long* NBT;                 // num_batches_tracked arena
  float* G;                       // gradient arena (backward)
  void* ws;                       // forward workspace (persists until backward)
  void* bws;                      // backward workspace
  const void* dout;               // grad wrt out (backward)
  const void* daux;               // grad wrt aux_out (backward) or null
  unsigned long long seed;        // dropout seed
  float dropout_p;
  float momentum;
  hipStream_t st;
  // fused loss head: forward with target != null computes the CE loss into loss2[0..1]
  // (mean, count) instead of writing full-resolution logits; backward with gloss != null
  // starts from d(loss) instead of d(logits).
  const long long* target = nullptr;
  long long ignore_index = -1;
  float* loss2 = nullptr;
  const float* gloss = nullptr;
  // head kind of the fused loss head: HEAD_CE (above) or HEAD_DICE, the Dice / Focal+Dice
  // criteria (utils/loss.py:12-100).  Dice: forward writes the loss into loss2[0] and the sums
  // (I, S, T, F) into dice_stats; the coefficient planes live in head_ws
  // (dice_head_ws_bytes), which the backward reads again.
  int head = 0;
  float smooth = 1e-6f, dice_weight = 1.f, focal_weight = 0.f, alpha = 0.5f, gamma = 2.f;
  void* head_ws = nullptr;
  double* dice_stats = nullptr;
  // HEAD_OHEM (utils/loss.py:127-206): weighted CE over the labelled pixels whose label
  // probability is <= the OHEM threshold; loss2 = (weighted mean, sum of kept weights), so the
  // backward is the CE head's.  Caller-owned device buffers: the probability plane [N H W], the
  // threshold scalar, the two counters (zeroed inside the run) and the select's 2056-word scratch.
  float ohem_thresh = 0.7f;
  long long ohem_min_kept = 0;
  const float* ohem_weight = nullptr;
  float* ohem_prob = nullptr;
  float* ohem_thr = nullptr;
  unsigned long long* ohem_counts = nullptr;
  unsigned* ohem_work = nullptr;
  // aux loss heads (aux nets, fscnn_forward_loss_aux): with aux_loss != 0 the forward runs the
  // head `head` on the main and then on the aux low-res logits and writes loss3 = (main +
  // aux_weight * aux, main, aux); the backward scales the main head's gradient as above and the
  // aux head's, times aux_weight, straight into g_auxlog (no upsample backward).  The main head
  // keeps the plan's g_raw / head_part; everything else both heads need lives in head_ws
  // (aux_head_ws_bytes, AuxHeadWs), the (mean, count) pairs / Dice stats the backward reads
  // included -- loss3 is only an output.
  int aux_loss = 0;
  float* loss3 = nullptr;
  // eval prediction: forward with labels != null writes argmax(upsampled logits) instead of out
  void* labels = nullptr;
  int label_u8 = 0;
  // validation (inference plans): forward with validate != 0 ends in the fused eval head
  // (evalhead.hip) instead of the upsample: loss2[0] = the criterion (head, target, ignore_index /
  // the Dice scalars above) of the main output, plus aux_weight times that of the aux output when
  // aux_weight != 0 (aux nets); counts (or null) accumulates the SegmentationMetric counters of
  // argmax(main output); head_ws holds the partial records (eval_head_parts x 4 floats)
  int validate = 0;
  float aux_weight = 0.f;
  unsigned long long* counts = nullptr;
  // deployment tail (inference plans, square input): forward with e2e_ho > 0 ends in e2e_head
  // (e2e.hip) instead of the upsample: the logits resampled (align_corners=False) to
  // e2e_ho x e2e_wo, as probabilities / logits into e2e_probs and / or scaled labels into
  // e2e_labels
  int e2e_ho = 0, e2e_wo = 0, e2e_softmax = 0, e2e_pdtype = 0, e2e_scale = 1;
  void* e2e_probs = nullptr;
  unsigned char* e2e_labels = nullptr;
  // bird's-eye tail (bev.hip): with bev_rows != null the deployment tail is e2e_bev instead --
  // the lane mask (argmax * e2e_scale at e2e_ho x e2e_wo) warped by bev_m (view -> frame) to
  // bev_hb x bev_wb into bev_mask (or null) and its row table into bev_rows
  int bev_hb = 0, bev_wb = 0, bev_min_width = 1;
  double bev_m[9] = {};
  unsigned char* bev_mask = nullptr;
  int* bev_rows = nullptr;
  // overlay tail (overlay.hip): with ov.out != null the deployment tail is e2e_overlay instead --
  // the frames ov.frames (ov.N is taken from the plan) blended with the colour of the class at
  // the nearest pixel of the e2e_ho x e2e_wo output; ov.mask_out (or null) gets argmax * e2e_scale
  OverlayArgs ov = {};
  OverlayColors ov_colors = {};
  // backward: gradient of the input image, NCHW [N][3][H][W] in dx_dtype (autograd of x through
  // conv0, models/fast_scnn.py:153), or null
  void* dx = nullptr;
  int dx_dtype = 0;
};

// Layout of the aux loss heads' caller buffer (byte offsets, 256-B aligned; index 0 = main head,
// 1 = aux head).  pair: the head's (mean, count) output, Dice: its loss scalar.  g_raw / part:
// the aux head's CE / OHEM gradient planes and partials (the main head uses the plan's).  dice /
// stats: each Dice head's coefficient planes (dice_head_ws_bytes) and double[4] sums.  prob / thr /
// counts: each OHEM head's probability plane, threshold and counter pair; work: the select scratch.
struct AuxHeadWs {
  size_t pair[2] = {}, g_raw = 0, part = 0, dice[2] = {}, stats[2] = {}, prob[2] = {}, thr[2] = {},
         counts[2] = {}, work = 0, bytes = 0;
};
// false (fscnn_last_error set): not an aux train = 1 plan, or an unknown head
bool aux_head_ws(const Plan& pl, int head, AuxHeadWs& l);

int net_forward(const Plan& pl, const RunArgs& r);
int net_backward(const Plan& pl, const RunArgs& r, int stage_from, int stage_to);

}  // namespace fscnn
