// enflow_backward.hip -- training backward of the fused coupling flow on MI355X.
//
// Reverse-mode gradient of  loss = Alchemical_NLL(LFIntegrator(data))
// (enflow/flow/loss.py:21-24, enflow/flow/dynamics.py:10-24, enflow/nn/egcl.py,
// enflow/nn/argmax.py) with respect to every parameter, i.e. what the
// reference's `loss.backward()` (enflow/main.py:219-221) produces by autograd.
//
// Data flow (one stream, no host synchronisation):
//   forward (enflow_flow.hip) with a tape: per layer the layer-input state
//     (h, g, pos, vel), the message sums and Q, plus per-molecule pair counts;
//   nll_bwd_kernel: adjoints of the flow outputs and of log|detJ|;
//   pair_offsets_kernel: 32-aligned per-molecule row offsets of every layer;
//   per layer, last to first:
//     lf_layer_bwd_kernel (one workgroup per molecule, state in LDS):
//       leapfrog adjoint -> node MLP backward (VALU, atoms x hidden units)
//       -> per 32-pair tile the edge chain is recomputed and back-propagated
//       on v_mfma_f32_32x32x2_f32 (transposed weight fragments, accumulator
//       tiles chained as B operands exactly as in the forward), writing the
//       per-pair (input, output-gradient) rows every weight gradient needs;
//     outer_acc_kernel + reduce_part_kernel: every weight gradient of the
//       layer as dW = sum_rows DY^T X (chunked over rows, fixed-order reduce,
//       deterministic), written straight into the torch parameter layout;
//   argmax_bwd_kernel (+ its two weight gradients).
// All arithmetic is float32.

#define ENFLOW_BACKWARD_TU   // -DENFLOW_STAMPS_BWD stamps this file's kernels only (tools/stamps_bwd.py)
// The kernels (file map: DESIGN.md section 3c).  The code object holds the plain
// kernels in the order these headers define them, then the template instances in
// the order the host code below first names them.
#include "enflow_bwd_layer.h"
#include "enflow_bwd_prep.h"
#include "enflow_bwd_wgrad.h"
#include "enflow_bwd_aux.h"
#include <stdlib.h>
#include <mutex>
#include <vector>

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
static inline size_t al64(size_t x) { return (x + 63) & ~(size_t)63; }
static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// Workspace: the per-layer pair-row / atom-row / partial sections come in
// BWD_NBUF copies (`span` floats apart): layer l's weight-gradient pass (outer
// kernels, on an auxiliary stream) reads buffer l % BWD_NBUF while the layer
// backwards of l-1, l-2 write the others.  Three buffers let the layer chain
// run two layers ahead of the weight-gradient passes instead of waiting on
// each one (backward -2.7 %, profiles/r02/r02y_ab_nbuf.txt; +6.6 GB at the
// bench batch); the large-system path and single layers use two.
#ifndef BWD_NBUF
#define BWD_NBUF 3
#endif
static_assert(BWD_NBUF >= 2, "at least double buffered");
struct BwdWs {
  size_t offs, buf0, span;   // shared offsets section; first buffer; buffer stride
  // offsets within a buffer (floats)
  size_t xin, pe, dp0, dpe, aphi, patt, dlogit, tmax, su, au, sn, an, aq, agr, anet, part, total;
  int nbuf;                  // buffers rotated by the layer chain (BWD_NBUF or 2)
  size_t part_floats;
};

static BwdWs bwd_ws(int num_mols, int num_atoms, int nf, int H, int n_layers, long long prb, int nbuf_cap = BWD_NBUF) {
  BwdWs W;
  size_t o = 0;
  const size_t P = (size_t)prb, A = (size_t)num_atoms;
  W.offs = 0;
  W.buf0 = al64((size_t)n_layers * (num_mols + 1));
  W.xin = o; o += al64(P * xin_width(nf));
  W.pe = o; o += al64(P * H);
  W.dp0 = o; o += al64(P * H);
  W.dpe = o; o += al64(P * H);
  W.aphi = o; o += al64(P);
  W.patt = o; o += al64(P);
  W.dlogit = o; o += al64(P);
  W.tmax = o; o += al64((P / 32 + 1) * TMX_W);
  W.su = o; o += al64(A * H);
  W.au = o; o += al64(A * H);
  W.sn = o; o += al64(A * H);
  W.an = o; o += al64(A * H);
  W.aq = o; o += al64(A);
  W.agr = o; o += al64(A * nf);
  W.anet = o; o += al64(A * 2 * nf);
  const size_t chp = (size_t)cdiv(prb, OA_CHUNK), cha = (size_t)cdiv(num_atoms, OA_CHUNK_ATOM);
  // partials of one layer's 8 gradients (all in flight together)
  W.part_floats = chp * ((size_t)H * (2 * nf + 2) + 2 * (size_t)H * (H + 1) + H + (H + 1)) +   // + att_nn
                  cha * ((size_t)H * (nf + 1) + (H + 1) + (size_t)H * (H + nf + 1) + (size_t)nf * (H + 1));
  const size_t am = cha * ((size_t)H * (nf + 1) + (size_t)2 * nf * (H + 1));
  if (am > W.part_floats) W.part_floats = am;
  W.part = o; o += al64(W.part_floats);
  W.span = o;
  // fused layer chains of >= BWD_NBUF layers rotate BWD_NBUF buffers; the
  // large-system path (n_layers 0 here) and single-layer callers use two
  W.nbuf = n_layers >= nbuf_cap ? nbuf_cap : 2;
  W.total = W.buf0 + (size_t)W.nbuf * W.span;
  return W;
}

// Auxiliary stream (per device) for the weight-gradient passes, and a pool of
// sync events.  Host-side state only; guarded by a mutex (one backward's launch
// sequence at a time per process).
namespace {
struct AuxDev {
  hipStream_t s = nullptr;
  std::vector<hipEvent_t> ev;
};
std::mutex g_aux_mu;
AuxDev g_aux[64];
hipStream_t aux_stream(int dev) {
  if (!g_aux[dev].s) {   // created on `dev` (the caller's stream's device)
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) return nullptr;
    if (cur != dev && hipSetDevice(dev) != hipSuccess) return nullptr;
    if (hipStreamCreateWithFlags(&g_aux[dev].s, hipStreamNonBlocking) != hipSuccess) g_aux[dev].s = nullptr;
    if (cur != dev) (void)hipSetDevice(cur);
  }
  return g_aux[dev].s;
}
hipEvent_t aux_event(int dev, size_t i) {
  auto& v = g_aux[dev].ev;
  while (v.size() <= i) {
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
    v.push_back(e);
  }
  return v[i];
}

// The weight-gradient pipeline of one backward call.  The layer
// chain runs on the caller's stream, last layer first; layer l's weight-gradient
// pass runs on aux() and reads the pair-row buffer the layer's backward wrote.
// Event 2 l: layer l's backward is done; event 2 l + 1: its pass is done.
//   wait_free(l, depth)  before layer l's backward: the caller's stream waits for the
//                        pass that last read its buffer (layer l + depth's; `depth` rotate)
//   layer_queued(l)      after it: event 2 l recorded, the auxiliary stream waits for it
//   grads_queued(l)      after the pass: event 2 l + 1 recorded; under ENFLOW_SERIAL_BWD
//                        (diagnostic: no overlap) the caller's stream waits for it at once
//   join()               after layer 0: the caller's stream waits for event 1, the last pass
// Holds g_aux_mu for its lifetime; false is a HIP failure (-2; nothing is joined then).
class AuxPipe {
 public:
  AuxPipe(hipStream_t st, int n_layers)
      : lock_(g_aux_mu), st_(st), n_(n_layers), serial_(getenv("ENFLOW_SERIAL_BWD") != nullptr) {
    if ((st ? hipStreamGetDevice(st, &dev_) : hipGetDevice(&dev_)) != hipSuccess || dev_ < 0 || dev_ >= 64) return;
    st2_ = aux_stream(dev_);
    for (int i = 0; st2_ && i < 2 * n_; ++i)
      if (!aux_event(dev_, (size_t)i)) st2_ = nullptr;
  }
  bool ok() const { return st2_ != nullptr; }
  hipStream_t aux() const { return st2_; }
  bool wait_free(int l, int depth) {
    return l + depth >= n_ || hipStreamWaitEvent(st_, ev(2 * (l + depth) + 1), 0) == hipSuccess;
  }
  bool layer_queued(int l) {
    return hipEventRecord(ev(2 * l), st_) == hipSuccess && hipStreamWaitEvent(st2_, ev(2 * l), 0) == hipSuccess;
  }
  bool grads_queued(int l) {
    if (hipEventRecord(ev(2 * l + 1), st2_) != hipSuccess) return false;
    return !serial_ || hipStreamWaitEvent(st_, ev(2 * l + 1), 0) == hipSuccess;
  }
  bool join() { return n_ <= 0 || hipStreamWaitEvent(st_, ev(1), 0) == hipSuccess; }

 private:
  hipEvent_t ev(int i) const { return g_aux[dev_].ev[(size_t)i]; }
  std::lock_guard<std::mutex> lock_;
  hipStream_t st_, st2_ = nullptr;
  int dev_ = 0, n_;
  bool serial_;
};
}  // namespace

// What one backward call passes around: the arguments of the fused, large,
// standalone-EGCL, list and reverse paths under one set of names.  Each extern
// "C" entry fills it once, by field name; what a path does not have stays null.
struct BwdCall {
  int num_mols = 0, num_atoms = 0, max_mol_atoms = 0, nf = 0, H = 0, n_layers = 0;
  const int32_t *mol_ptr = nullptr, *pair_counts = nullptr;
  const float *r_cut = nullptr, *box = nullptr, *tape = nullptr;
  const float *layers = nullptr, *layers_bwd = nullptr, *layers_raw = nullptr;   // forward / backward / raw sections
  const float *dequant_raw = nullptr, *h_data = nullptr, *noise = nullptr;        // the dequantiser's inputs
  float dt = 0.f, cw = 0.f;
  float *adj_h = nullptr, *adj_g = nullptr, *adj_pos = nullptr, *adj_vel = nullptr;
  const float* adj_ldj = nullptr;
  float *grad_layers = nullptr, *grad_dequant = nullptr;
  void* workspace = nullptr;
  int64_t workspace_bytes = 0, pair_row_bound = 0;
  int32_t* err_flag = nullptr;
  hipStream_t stream = nullptr;
  const float *eg_dQ = nullptr, *eg_dF = nullptr, *eg_dG = nullptr;   // standalone EGCL: the adjoints of Q, F, G
  int kind = ENFLOW_DEQUANT_NONE;        // the dequantiser, and what else its word carried (decode_flags):
  bool variants = false, f32b = false;   // layers with variant flags; the fp32 backward
  bool ldj_atoms = false;                // ENFLOW_BWD_LDJ_ATOMS: adj_ldj holds one value per atom, else one float
};

// A flow entry's dequant_kind carries ENFLOW_EGCL_VARIANTS (layers with
// norm_diff / tanh flags) and ENFLOW_BWD_F32 (the tape of an fp32-GEMM forward:
// fp32 backward) above the dequantiser's kind; a standalone layer's egcl_flags
// carry its own flags in the low byte instead (no dequantiser) and ENFLOW_BWD_F32.
// ENFLOW_BWD_LDJ_ATOMS (flow entries only): adj_ldj is [num_atoms], not one float.
static void decode_flags(BwdCall& c, int word, bool egcl_flags) {
  c.variants = egcl_flags ? (word & 0xff) != 0 : (word & ENFLOW_EGCL_VARIANTS) != 0;
  c.f32b = (word & ENFLOW_BWD_F32) != 0;
  c.ldj_atoms = !egcl_flags && (word & ENFLOW_BWD_LDJ_ATOMS) != 0;
  c.kind = egcl_flags ? ENFLOW_DEQUANT_NONE : (word & 0xff);
}

static void add_desc(OuterBatch& ob, const float* DY, int ldd, int M, const float* X, int ldx, int N,
                     const int32_t* rows_dev, int rows_static, int rows_bound, float*& part, float* outW,
                     float* outB, int tiled = 0) {
  OuterDesc& D = ob.d[ob.nd];
  D.tiled = tiled;
  D.xf_x = 0;
  D.xrow = nullptr;
  D.xf_dy = 0;
  D.rowv = nullptr;
  D.colv = nullptr;
  D.part2 = nullptr;
  D.recomp = RECOMP_NONE;
  D.Lp = nullptr;
  D.nf = 0;
  D.actp = nullptr;
  D.f32r = 0;
  D.tmaxA = D.tmaxB = nullptr;
  D.chunk = tiled ? OA_CHUNK : OA_CHUNK_ATOM;
  D.DY = DY; D.ldd = ldd; D.M = M; D.X = X; D.ldx = ldx; D.N = N;
  D.rows_dev = rows_dev; D.rows_static = rows_static;
  D.outW = outW; D.outB = outB;
  D.mb = 1;
  D.nb = cdiv(N, 128);
  D.nch = rows_bound > 0 ? cdiv(rows_bound, D.chunk) : 0;
  D.part = part;
  part += (size_t)D.nch * M * (N + (outB ? 1 : 0));
  // the descriptor's workgroups follow those of the descriptors before it
  const int wg = ob.nd ? ob.start[ob.nd] : 0;
  ob.start[ob.nd] = wg;
  ++ob.nd;
  ob.start[ob.nd] = wg + D.nch * D.nb;
}

static int run_outer(OuterBatch& ob, hipStream_t st) {
  // one launch per layout (tile-blocked pair rows / row-major atom rows)
  for (int tl = 0; tl < 2; ++tl) {
    OuterBatch sub;
    sub.nd = 0;
    int swg = 0;
    for (int k = 0; k < ob.nd; ++k) {
      if (ob.d[k].tiled != tl) continue;
      sub.d[sub.nd] = ob.d[k];
      sub.start[sub.nd] = swg;
      swg += ob.start[k + 1] - ob.start[k];
      sub.start[++sub.nd] = swg;
    }
    if (swg > 0) {
      bool gen = false;   // a non-SiLU act_fn in the batch: the generic-activation instance
      for (int k = 0; k < sub.nd; ++k) gen |= sub.d[k].actp != nullptr;
      if (tl && gen) ENFLOW_TIMED("outer_acc_kernel", st, hipLaunchKernelGGL((outer_acc_kernel<true, true>), dim3(swg), dim3(256), 0, st, sub));
      else if (tl) ENFLOW_TIMED("outer_acc_kernel", st, hipLaunchKernelGGL((outer_acc_kernel<true, false>), dim3(swg), dim3(256), 0, st, sub));
      else ENFLOW_TIMED("outer_acc_kernel", st, hipLaunchKernelGGL((outer_acc_kernel<false, false>), dim3(swg), dim3(256), 0, st, sub));
    }
  }
  // F16X3 MFMA: tile-blocked descriptors with M > 1
  {
    OuterBatch sub;
    sub.nd = 0;
    int swg = 0;
    for (int k = 0; k < ob.nd; ++k) {
      if (ob.d[k].tiled != 2) continue;
      sub.d[sub.nd] = ob.d[k];
      sub.start[sub.nd] = swg;
      swg += ob.start[k + 1] - ob.start[k];
      sub.start[++sub.nd] = swg;
    }
    bool gen = false, f32r = false;
    for (int k = 0; k < sub.nd; ++k) {
      gen |= sub.d[k].actp != nullptr;
      f32r |= sub.d[k].f32r != 0;
    }
    if (swg > 0 && f32r) ENFLOW_TIMED("outer_x3_kernel", st, hipLaunchKernelGGL((outer_x3_kernel<true, true>), dim3(swg), dim3(256), 0, st, sub));
    else if (swg > 0 && gen) ENFLOW_TIMED("outer_x3_kernel", st, hipLaunchKernelGGL(outer_x3_kernel<true>, dim3(swg), dim3(256), 0, st, sub));
    else if (swg > 0) ENFLOW_TIMED("outer_x3_kernel", st, hipLaunchKernelGGL(outer_x3_kernel<false>, dim3(swg), dim3(256), 0, st, sub));
  }
  // reducer: one workgroup per 256 outputs of each descriptor
  OuterBatch rb = ob;
  int rw = 0;
  for (int k = 0; k < ob.nd; ++k) {
    rb.start[k] = rw;
    const int NB = ob.d[k].N + (ob.d[k].outB ? 1 : 0);
    rw += cdiv((long long)ob.d[k].M * NB, RP_OUT);
  }
  rb.start[ob.nd] = rw;
  if (rw > 0) ENFLOW_TIMED("reduce_part_kernel", st, hipLaunchKernelGGL(reduce_part_kernel, dim3(rw), dim3(256), 0, st, rb));
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// Layer l's weight gradients from its pair rows (prow: device count of pair
// rows) and atom rows in buffer wb, straight into the torch parameter layout
// (the layer's slice of grad_layers), on stream st2.
static int layer_weight_grads(const BwdCall& c, int l, hipStream_t st2, const BwdWs& Wl, float* wb,
                              const int32_t* prow) {
    const int num_atoms = c.num_atoms, nf = c.nf, H = c.H, prb = (int)c.pair_row_bound;
    const bool variants = c.variants, f32b = c.f32b;
    const RawEgcl R = raw_egcl(H, nf);
    float* G = c.grad_layers + (size_t)l * R.total_bwd;
    const float *Rp = c.layers_raw + (size_t)l * R.total_bwd, *Lp = c.layers + (size_t)l * egcl_layout(H, nf).total;
    const float* hx = c.tape + tape_layout(num_atoms, nf, H, c.n_layers).hx + (size_t)l * num_atoms * (nf + H);
    OuterBatch ob;
    ob.nd = 0;
    float* part = wb + Wl.part;
    const int XW = xin_width(nf);
    add_desc(ob, wb + Wl.dp0, H, H, wb + Wl.xin, XW, 2 * nf + 1, prow, 0, prb, part, G + R.We1, G + R.be1,
             2);   // tiled 2: outer_x3_kernel
    ob.d[ob.nd - 1].tmaxA = wb + Wl.tmax + TMX_DP0;
    ob.d[ob.nd - 1].tmaxB = wb + Wl.tmax + TMX_XIN;
    // edge_nn.2: X = silu(pre0), pre0 recomputed from the xin rows
    // the layer's act_fn (variant layers; packed layer + vfl + 1): the recomputed
    // activations and their derivatives follow it (NULL: SiLU instances)
    // (the fp32 backward always runs the generic instances)
    const float* actp = (variants || f32b) ? Lp + egcl_layout(H, nf).vfl + 1 : nullptr;
    add_desc(ob, wb + Wl.dpe, H, H, wb + Wl.xin, XW, H, prow, 0, prb, part, G + R.We2, G + R.be2, 2);
    ob.d[ob.nd - 1].recomp = RECOMP_X0;
    ob.d[ob.nd - 1].tmaxA = wb + Wl.tmax + TMX_DPE;
    ob.d[ob.nd - 1].tmaxB = wb + Wl.tmax + TMX_X1;
    ob.d[ob.nd - 1].Lp = Lp;
    ob.d[ob.nd - 1].nf = nf;
    ob.d[ob.nd - 1].actp = actp;
    ob.d[ob.nd - 1].f32r = f32b;
    // coord_nn.0: X = silu(pre_e) = the message; DY = aphi * wc2 * silu'(pc), pc recomputed from X
    add_desc(ob, nullptr, H, H, wb + Wl.pe, H, H, prow, 0, prb, part,
             G + R.Wc1, G + R.bc1, 2);
    ob.d[ob.nd - 1].xf_x = 1;
    ob.d[ob.nd - 1].xf_dy = 1;
    ob.d[ob.nd - 1].rowv = wb + Wl.aphi;
    if (variants) ob.d[ob.nd - 1].xrow = wb + Wl.patt;          // the message is e * att
    ob.d[ob.nd - 1].colv = Rp + R.wc2;
    ob.d[ob.nd - 1].recomp = RECOMP_PC;
    ob.d[ob.nd - 1].tmaxA = wb + Wl.tmax + TMX_DPC;
    ob.d[ob.nd - 1].tmaxB = wb + Wl.tmax + TMX_MSG;
    ob.d[ob.nd - 1].Lp = Lp;
    ob.d[ob.nd - 1].nf = nf;
    ob.d[ob.nd - 1].actp = actp;
    ob.d[ob.nd - 1].f32r = f32b;
    // coord_nn.2: d wc2 = sum_rows aphi silu(pc), folded into coord_nn.0's pass (its partials
    // written there; this descriptor only sizes them and feeds the reduction)
    add_desc(ob, wb + Wl.aphi, 1, 1, nullptr, H, H, prow, 0, prb, part, G + R.wc2, nullptr, 3);
    ob.d[ob.nd - 2].part2 = ob.d[ob.nd - 1].part;
    if (variants) {   // att_nn.0: d w = sum_rows dlogit e, d b = sum_rows dlogit (0 rows without attention)
      add_desc(ob, wb + Wl.dlogit, 1, 1, wb + Wl.pe, H, H, prow, 0, prb, part, G + R.watt, G + R.batt, 1);
      ob.d[ob.nd - 1].xf_x = 1;                                 // X = silu(pre_e) = e
      ob.d[ob.nd - 1].actp = actp;
    }
    add_desc(ob, wb + Wl.au, H, H, hx, nf + H, nf, nullptr, num_atoms, num_atoms, part, G + R.Wv1, G + R.bv1);
    add_desc(ob, wb + Wl.aq, 1, 1, wb + Wl.su, H, H, nullptr, num_atoms, num_atoms, part, G + R.Wv2, G + R.bv2);
    add_desc(ob, wb + Wl.an, H, H, hx, nf + H, nf + H, nullptr, num_atoms, num_atoms, part, G + R.Wn1,
             G + R.bn1);
    add_desc(ob, wb + Wl.agr, nf, nf, wb + Wl.sn, H, H, nullptr, num_atoms, num_atoms, part, G + R.Wn2,
             G + R.bn2);
    return run_outer(ob, st2);
}

// ArgMax.network's gradients (the flow's dequantiser) into grad_dequant; ptr /
// chunks: the atom chunks argmax_bwd_kernel runs on (<= nmax_sel atoms each)
static int argmax_grads(const BwdCall& c, const BwdWs& Wl, float* wb, const int32_t* ptr, int chunks, int nmax_sel) {
    const hipStream_t st = c.stream;
    const int H = c.H, nf = c.nf, num_atoms = c.num_atoms;
    const float *h_data = c.h_data, *noise = c.noise, *dequant_raw = c.dequant_raw, *adj_h = c.adj_h, *adj_ldj = c.adj_ldj;
    float* grad_dequant = c.grad_dequant;
    float* apre = wb + Wl.au;
    float* spre = wb + Wl.su;
    float* anet = wb + Wl.anet;
    if (c.ldj_atoms)
      launch_argmax_bwd_ldja(H, nmax_sel, chunks, st, ptr, nf, h_data, noise, dequant_raw, adj_h, adj_ldj, apre, spre,
                             anet);
    else argmax_bwd_launch(H, nmax_sel, chunks, st, ptr, nf, h_data, noise, dequant_raw, adj_h, adj_ldj, apre, spre, anet);
    const int rW1 = 0, rb1 = H * nf, rW2 = rb1 + H, rb2 = rW2 + 2 * nf * H;
    OuterBatch ob;
    ob.nd = 0;
    float* part = wb + Wl.part;
    add_desc(ob, apre, H, H, h_data, nf, nf, nullptr, num_atoms, num_atoms, part, grad_dequant + rW1,
             grad_dequant + rb1);
    add_desc(ob, anet, 2 * nf, 2 * nf, spre, H, H, nullptr, num_atoms, num_atoms, part, grad_dequant + rW2,
             grad_dequant + rb2);
    return run_outer(ob, st);
}

extern "C" {

#if defined(ENFLOW_STAMPS_BWD) && !defined(ENFLOW_STAMPS)
int enflow_read_stamps(unsigned long long* host_out, int reset) {
  if (hipMemcpyFromSymbol(host_out, HIP_SYMBOL(enflow_stamp_acc), sizeof(unsigned long long) * NSTAMP) != hipSuccess)
    return -2;
  if (reset) {
    unsigned long long z[NSTAMP] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(enflow_stamp_acc), z, sizeof(z)) != hipSuccess) return -2;
  }
  return NSTAMP;
}
#endif

int64_t enflow_lf_tape_size(int num_atoms, int nf, int H, int n_layers) {
  if (num_atoms < 0 || nf < 1 || nf > BWD_NFMAX || !hid_ok(H) || n_layers < 0) return -1;
  return (int64_t)tape_layout(num_atoms, nf, H, n_layers).total;
}

// The neighbour-list section (pair words and row counts, the layout's tail) is
// written by the 33..64-atom fused forward and read back by its backward only;
// other batches' tapes end before it.
int64_t enflow_lf_tape_size_for(int num_atoms, int nf, int H, int n_layers, int max_mol_atoms) {
  if (num_atoms < 0 || nf < 1 || nf > BWD_NFMAX || !hid_ok(H) || n_layers < 0 || max_mol_atoms < 0) return -1;
  const TapeLayout T = tape_layout(num_atoms, nf, H, n_layers);
  static_assert(TAPE_PAIR_CAP + 1 == 64, "the pair section belongs to the 64-atom instance");
  return (int64_t)(max_mol_atoms > 32 && max_mol_atoms <= TAPE_PAIR_CAP + 1 ? T.total : T.pairs);
}

int64_t enflow_egcl_bwd_packed_size(int H, int nf) {
  if (!hid_ok(H) || nf < 1 || nf > BWD_NFMAX) return -1;
  return egcl_bwd_layout(H).total;
}

int enflow_pack_egcl_bwd_f32(const float* raw, int H, int nf, float* packed, void* stream) {
  if (!hid_ok(H) || nf < 1 || nf > BWD_NFMAX || !raw || !packed) return -1;
  const int total = egcl_bwd_layout(H).total;
  hipLaunchKernelGGL(egcl_bwd_scale_kernel, dim3(6), dim3(256), 0, S(stream), raw, H, nf, packed);
  hipLaunchKernelGGL(pack_egcl_bwd_kernel, dim3(cdiv(total, 256)), dim3(256), 0, S(stream), raw, H, nf, packed);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int enflow_pack_egcl_bwd_layers_f32(const float* raw, int64_t raw_stride, int n_layers, int H, int nf,
                                    float* packed, void* stream) {
  if (!hid_ok(H) || nf < 1 || nf > BWD_NFMAX || !raw || !packed || n_layers < 0 || n_layers > 65535) return -1;
  if (raw_stride < raw_egcl(H, nf).total) return -1;
  if (n_layers == 0) return 0;
  const int total = egcl_bwd_layout(H).total;
  hipLaunchKernelGGL(egcl_bwd_scale_layers_kernel, dim3(6, n_layers), dim3(256), 0, S(stream), raw, raw_stride, H, nf,
                     packed, (int64_t)total);
  hipLaunchKernelGGL(pack_egcl_bwd_layers_kernel, dim3(cdiv(total, 256), n_layers), dim3(256), 0, S(stream), raw,
                     raw_stride, H, nf, packed, (int64_t)total);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int64_t enflow_lf_backward_workspace_size(int num_mols, int num_atoms, int nf, int H, int n_layers,
                                          int64_t pair_row_bound) {
  if (num_mols < 0 || num_atoms < 0 || nf < 1 || nf > BWD_NFMAX || !hid_ok(H) || n_layers < 0 || pair_row_bound < 0)
    return -1;
  return (int64_t)(bwd_ws(num_mols, num_atoms, nf, H, n_layers, pair_row_bound).total * sizeof(float));
}

int64_t enflow_lf_backward_workspace_size_min(int num_mols, int num_atoms, int nf, int H, int n_layers,
                                              int64_t pair_row_bound) {
  if (num_mols < 0 || num_atoms < 0 || nf < 1 || nf > BWD_NFMAX || !hid_ok(H) || n_layers < 0 || pair_row_bound < 0)
    return -1;
  return (int64_t)(bwd_ws(num_mols, num_atoms, nf, H, n_layers, pair_row_bound, 2).total * sizeof(float));
}

int enflow_alchemical_nll_backward_f32(int num_mols, int num_atoms, int max_mol_atoms, int nf,
                                       const int32_t* mol_ptr, const float* h, const float* g,
                                       const float* pos, const float* vel, float kBT, float softening,
                                       const float* grad_loss, float* adj_h, float* adj_g, float* adj_pos,
                                       float* adj_vel, float* adj_ldj, void* stream) {
  if (num_mols < 1 || num_atoms < 0 || nf < 1 || !adj_ldj) return -1;
  const int tm = enflow_tm_begin("nll_bwd_kernel", S(stream));
  if (max_mol_atoms > 64)
    hipLaunchKernelGGL(nll_bwd_large_kernel, dim3(num_atoms / WAVES + 1), dim3(BLOCK), 0, S(stream), mol_ptr,
                       num_mols, num_atoms, nf, h, g, pos, vel, kBT, softening, grad_loss, adj_h, adj_g, adj_pos,
                       adj_vel, adj_ldj);
  else if (max_mol_atoms <= 32)
    hipLaunchKernelGGL((nll_bwd_kernel<32>), dim3(num_mols), dim3(BLOCK), 0, S(stream), mol_ptr, num_mols, nf, h, g,
                       pos, vel, kBT, softening, grad_loss, adj_h, adj_g, adj_pos, adj_vel, adj_ldj);
  else
    hipLaunchKernelGGL((nll_bwd_kernel<64>), dim3(num_mols), dim3(BLOCK), 0, S(stream), mol_ptr, num_mols, nf, h, g,
                       pos, vel, kBT, softening, grad_loss, adj_h, adj_g, adj_pos, adj_vel, adj_ldj);
  enflow_tm_end(tm, S(stream));
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int enflow_alchemical_nll_mol_backward_f32(int num_mols, int num_atoms, int max_mol_atoms, int nf,
                                           const int32_t* mol_ptr, const float* h, const float* g,
                                           const float* pos, const float* vel, float softening,
                                           const float* grad_out, const float* coef, float* adj_h, float* adj_g,
                                           float* adj_pos, float* adj_vel, void* stream) {
  if (num_mols < 0 || num_atoms < 0 || max_mol_atoms < 0 || nf < 1 || nf > BWD_NFMAX) return -1;
  if (num_mols == 0 || num_atoms == 0) return 0;
  if (!mol_ptr || !pos || !grad_out || !coef || !adj_pos) return -1;
  if ((adj_h && !h) || (adj_g && !g) || (adj_vel && !vel)) return -1;
  NllCoef c;
  for (int k = 0; k < 4; ++k) c.c[k] = coef[k];
  const int tm = enflow_tm_begin("nll_mol_bwd_kernel", S(stream));
#define NLL_MOL_BWD(NN)                                                                                             \
  hipLaunchKernelGGL((nll_mol_bwd_kernel<NN>), dim3(num_mols), dim3(BLOCK), 0, S(stream), mol_ptr, nf, h, g, pos, \
                     vel, softening, grad_out, c, adj_h, adj_g, adj_pos, adj_vel)
  if (max_mol_atoms <= 32) NLL_MOL_BWD(32);
  else if (max_mol_atoms <= 64) NLL_MOL_BWD(64);
  else if (max_mol_atoms <= 256) NLL_MOL_BWD(256);
  else
    hipLaunchKernelGGL(nll_mol_bwd_large_kernel, dim3(cdiv(num_atoms, WAVES)), dim3(BLOCK), 0, S(stream), mol_ptr,
                       num_mols, num_atoms, nf, h, g, pos, vel, softening, grad_out, c, adj_h, adj_g, adj_pos,
                       adj_vel);
#undef NLL_MOL_BWD
  enflow_tm_end(tm, S(stream));
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// The BwdArgs fields the fused and the large-system backward set alike for layer
// l (wb: the layer's workspace buffer); each caller adds its own pair source.
static BwdArgs layer_bwd_args(const BwdCall& c, int l, float* wb, const BwdWs& Wl) {
  BwdArgs A{};
  A.mol_ptr = c.mol_ptr; A.r_cut = c.r_cut; A.box = c.box; A.tape = c.tape;
  A.num_atoms = c.num_atoms; A.num_mols = c.num_mols; A.n_layers = c.n_layers; A.layer = l; A.nf = c.nf;
  A.Lp = c.layers + (size_t)l * egcl_layout(c.H, c.nf).total;
  A.Bp = c.layers_bwd + (size_t)l * egcl_bwd_layout(c.H).total;
  A.Rp = c.layers_raw + (size_t)l * raw_egcl(c.H, c.nf).total_bwd;
  A.dt = c.dt; A.cw = c.cw; A.adj_ldj = c.adj_ldj;
  A.ah = c.adj_h; A.ag = c.adj_g; A.apos = c.adj_pos; A.avel = c.adj_vel;
  A.xin = wb + Wl.xin; A.pe = wb + Wl.pe;
  A.dp0 = wb + Wl.dp0; A.dpe = wb + Wl.dpe; A.aphi = wb + Wl.aphi;
  A.patt = wb + Wl.patt; A.dlogit = wb + Wl.dlogit; A.tmax = wb + Wl.tmax;
  A.su = wb + Wl.su; A.au = wb + Wl.au; A.sn = wb + Wl.sn; A.an = wb + Wl.an;
  A.aq = wb + Wl.aq; A.agr = wb + Wl.agr; A.err = c.err_flag;
  A.eg_dQ = c.eg_dQ; A.eg_dF = c.eg_dF; A.eg_dG = c.eg_dG;
  return A;
}

// The final launch of a backward: a set error word leaves NaN in every weight
// gradient (and ArgMax.network's: W1, b1, W2, b2).
static int poison_grads(const BwdCall& c) {
  const long long argmax_len = (long long)(c.H * c.nf + c.H + 2 * c.nf * c.H + 2 * c.nf);
  hipLaunchKernelGGL(poison_on_err_kernel, dim3(64), dim3(256), 0, c.stream, c.err_flag, c.grad_layers,
                     (long long)c.n_layers * raw_egcl(c.H, c.nf).total_bwd,
                     c.kind == ENFLOW_DEQUANT_ARGMAX ? c.grad_dequant : nullptr, argmax_len);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// lf_layer_bwd_kernel of one layer (layer_bwd_launch, enflow_bwd_layer.h).
// ldja: the ENFLOW_BWD_LDJ_ATOMS instances (adj_ldj per atom), enflow_backward_ldja.hip's.
static void launch_layer_bwd(int H, int nmax, bool big, bool f32b, bool variants, bool ldja, int grid, hipStream_t st,
                             const BwdArgs& A) {
  if (ldja) return launch_layer_bwd_ldja(H, nmax, big, f32b, variants, grid, st, A);
  layer_bwd_launch(H, nmax, big, f32b, variants, grid, st, A);
}

static int lf_backward_impl(const BwdCall& c) {
  const int num_mols = c.num_mols, num_atoms = c.num_atoms, nf = c.nf, H = c.H, n_layers = c.n_layers;
  if (num_mols < 0 || num_atoms < 0 || c.max_mol_atoms < 0 || c.max_mol_atoms > 64 || nf < 1 || nf > BWD_NFMAX ||
      !hid_ok(H) || n_layers < 0 || c.pair_row_bound < 0 || c.pair_row_bound > 0x7fffffffLL)
    return -1;
  if (!c.tape || !c.pair_counts || !c.layers || !c.layers_bwd || !c.layers_raw || !c.adj_h || !c.adj_g ||
      !c.adj_pos || !c.adj_vel || !c.adj_ldj || !c.grad_layers || !c.workspace || !c.err_flag)
    return -1;
  if (c.kind == ENFLOW_DEQUANT_ARGMAX && (!c.dequant_raw || !c.h_data || !c.noise || !c.grad_dequant)) return -1;
  // BWD_NBUF rotating buffers when the workspace holds them, else two (the
  // layer chain then waits for the weight-gradient pass two layers up)
  BwdWs Wl = bwd_ws(num_mols, num_atoms, nf, H, n_layers, c.pair_row_bound);
  if ((uint64_t)c.workspace_bytes < Wl.total * sizeof(float)) Wl = bwd_ws(num_mols, num_atoms, nf, H, n_layers, c.pair_row_bound, 2);
  if ((uint64_t)c.workspace_bytes < Wl.total * sizeof(float)) return -6;
  if (num_mols == 0) return 0;
  hipStream_t st = c.stream;
  float* ws = reinterpret_cast<float*>(c.workspace);
  int32_t* offs = reinterpret_cast<int32_t*>(ws + Wl.offs);
  // weight-gradient passes of layer l run on an auxiliary stream, overlapping the
  // layer backward of l - 1 (rotating rows); the caller's stream joins it
  // before the dequantiser's gradients and before returning
  AuxPipe pipe(st, n_layers);
  if (!pipe.ok()) return -2;

  if (n_layers > 0)
    hipLaunchKernelGGL(pair_offsets_kernel, dim3(n_layers), dim3(BLOCK), 0, st, c.pair_counts, num_mols, offs);

  for (int l = n_layers - 1; l >= 0; --l) {
    float* const wb = ws + Wl.buf0 + (size_t)(l % Wl.nbuf) * Wl.span;   // this layer's buffer
    if (!pipe.wait_free(l, Wl.nbuf)) return -2;
    BwdArgs A = layer_bwd_args(c, l, wb, Wl);
    A.pair_off = offs + (size_t)l * (num_mols + 1);
    A.pair_counts_l = c.pair_counts + (size_t)l * num_mols;
    // the forward's 64-atom instance tapes the list (molecules of 33..64 atoms; see flow_kernel.h)
    A.tape_pairs = c.eg_dQ == nullptr && c.max_mol_atoms > 32 && !getenv("ENFLOW_BWD_REBUILD_PAIRS");
    launch_layer_bwd(H, c.max_mol_atoms, false, c.f32b, c.variants, c.ldj_atoms, num_mols, st, A);
    if (!pipe.layer_queued(l)) return -2;
    const int rc = layer_weight_grads(c, l, pipe.aux(), Wl, wb, offs + (size_t)l * (num_mols + 1) + num_mols);
    if (rc) return rc;
    if (!pipe.grads_queued(l)) return -2;
  }
  // every weight-gradient pass done before the dequantiser's (buffer 0 again) and the return
  if (!pipe.join()) return -2;

  if (c.kind == ENFLOW_DEQUANT_ARGMAX) {
    const int rc = argmax_grads(c, Wl, ws + Wl.buf0, c.mol_ptr, num_mols, c.max_mol_atoms);
    if (rc) return rc;
  }
  return poison_grads(c);
}

int enflow_lf_backward_f32(int num_mols, int num_atoms, int max_mol_atoms, int nf, int H,
                           const int32_t* mol_ptr, const float* r_cut, const float* box,
                           const float* tape, const int32_t* pair_counts,
                           const float* layers, const float* layers_bwd, const float* layers_raw, int n_layers,
                           int dequant_kind, const float* dequant_raw, const float* h_data, const float* noise,
                           float dt, float cw,
                           float* adj_h, float* adj_g, float* adj_pos, float* adj_vel, const float* adj_ldj,
                           float* grad_layers, float* grad_dequant,
                           void* workspace, int64_t workspace_bytes, int64_t pair_row_bound,
                           int32_t* err_flag, void* stream) {
  BwdCall c;
  c.num_mols = num_mols; c.num_atoms = num_atoms; c.max_mol_atoms = max_mol_atoms; c.nf = nf; c.H = H;
  c.n_layers = n_layers; c.mol_ptr = mol_ptr; c.r_cut = r_cut; c.box = box; c.tape = tape; c.pair_counts = pair_counts;
  c.layers = layers; c.layers_bwd = layers_bwd; c.layers_raw = layers_raw; c.dt = dt; c.cw = cw;
  c.dequant_raw = dequant_raw; c.h_data = h_data; c.noise = noise; c.grad_dequant = grad_dequant;
  c.adj_h = adj_h; c.adj_g = adj_g; c.adj_pos = adj_pos; c.adj_vel = adj_vel; c.adj_ldj = adj_ldj;
  c.grad_layers = grad_layers; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
  c.pair_row_bound = pair_row_bound; c.err_flag = err_flag; c.stream = S(stream);
  decode_flags(c, dequant_kind, false);
  return lf_backward_impl(c);
}

int enflow_ldj_mol_to_atoms_f32(int num_mols, int num_atoms, const int32_t* mol_ptr, const float* adj_ldj_mol,
                                float* adj_ldj_atoms, void* stream) {
  if (num_mols < 0 || num_atoms < 0) return -1;
  if (num_mols == 0 || num_atoms == 0) return 0;
  if (!mol_ptr || !adj_ldj_mol || !adj_ldj_atoms) return -1;
  ENFLOW_TIMED("ldj_mol_to_atoms_kernel", S(stream),
               hipLaunchKernelGGL(ldj_mol_to_atoms_kernel, dim3(cdiv(num_atoms, BLOCK)), dim3(BLOCK), 0, S(stream),
                                  mol_ptr, num_mols, num_atoms, adj_ldj_mol, adj_ldj_atoms));
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// ---- large systems (molecules past the fused backward's 64-atom image) -----
// Per layer, last to first: the neighbour list of the layer's taped positions
// (the forward's own search kernels, + the dense slot map), the pair-row offsets
// of the row blocks, lf_layer_bwd_kernel<.., BIG> per block of rows (row-side
// adjoints in LDS, column-side per pair into colc), the column sums (colsum per
// row chunk, colfinal per id_mapping label), then the weight gradients on the
// auxiliary stream as in the fused backward.
struct LgBwdWs { size_t lg, smap, bwd, colc, part, boff, tot, rowstart, chunk, total; int nch, nb; };
static LgBwdWs lg_bwd_ws(int num_mols, int num_atoms, int max_n, int nf, int H, long long prb) {
  LgBwdWs W;
  const size_t A = (size_t)num_atoms;
  W.nch = max(1, cdiv(max_n, LG_RC));
  W.nb = num_atoms / lg_rows(num_atoms) + num_mols + 1;
  size_t o = 0;
  W.lg = o; o = al256(o + lg_workspace(num_mols, num_atoms, max_n, nf).total);
  W.smap = o; o = al256(o + A * (size_t)max_n * 4);
  W.bwd = o; o = al256(o + bwd_ws(num_mols, num_atoms, nf, H, 0, prb).total * sizeof(float));
  W.colc = o; o = al256(o + (size_t)prb * CSTR * 4);
  W.part = o; o = al256(o + (size_t)W.nch * A * CSTR * 4);
  W.boff = o; o = al256(o + 2 * ((size_t)W.nb + 1) * 4);
  W.tot = o; o = al256(o + 2 * 4);
  W.rowstart = o; o = al256(o + A * 4);
  W.chunk = o; o = al256(o + ((A + 31) / 32 + 2) * 4);
  W.total = o;
  return W;
}

int64_t enflow_lf_backward_large_workspace_size(int num_mols, int num_atoms, int max_mol_atoms, int nf, int H,
                                                int64_t pair_row_bound) {
  if (num_mols < 0 || num_atoms < 0 || max_mol_atoms < 0 || max_mol_atoms >= (1 << 22) || nf < 1 || nf > BWD_NFMAX ||
      !hid_ok(H) || pair_row_bound < 0 || pair_row_bound > 0x7fffffffLL)
    return -1;
  return (int64_t)lg_bwd_ws(num_mols, num_atoms, max_mol_atoms, nf, H, pair_row_bound).total;
}

static int lf_backward_large_impl(const BwdCall& c) {
  const int num_mols = c.num_mols, num_atoms = c.num_atoms, max_mol_atoms = c.max_mol_atoms, nf = c.nf, H = c.H,
            n_layers = c.n_layers;
  const int64_t need = enflow_lf_backward_large_workspace_size(num_mols, num_atoms, max_mol_atoms, nf, H,
                                                               c.pair_row_bound);
  if (need < 0 || n_layers < 0) return -1;
  if (!c.mol_ptr || !c.r_cut || !c.box || !c.tape || !c.layers || !c.layers_bwd || !c.layers_raw || !c.adj_h ||
      !c.adj_g || !c.adj_pos || !c.adj_vel || !c.adj_ldj || !c.grad_layers || !c.workspace || !c.err_flag)
    return -1;
  if (c.kind == ENFLOW_DEQUANT_ARGMAX && (!c.dequant_raw || !c.h_data || !c.noise || !c.grad_dequant)) return -1;
  if (c.workspace_bytes < need) return -6;
  if (num_mols == 0) return 0;
  const LgBwdWs W = lg_bwd_ws(num_mols, num_atoms, max_mol_atoms, nf, H, c.pair_row_bound);
  const BwdWs Wl = bwd_ws(num_mols, num_atoms, nf, H, 0, c.pair_row_bound);   // two buffers
  char* base = static_cast<char*>(c.workspace);
  float* ws = reinterpret_cast<float*>(base + W.bwd);
  int32_t* smap = reinterpret_cast<int32_t*>(base + W.smap);
  float* colc = reinterpret_cast<float*>(base + W.colc);
  float* part = reinterpret_cast<float*>(base + W.part);
  int32_t* boff = reinterpret_cast<int32_t*>(base + W.boff);
  int32_t* tot = reinterpret_cast<int32_t*>(base + W.tot);
  int32_t* rowstart = reinterpret_cast<int32_t*>(base + W.rowstart);
  int32_t* chunk = reinterpret_cast<int32_t*>(base + W.chunk);
  hipStream_t st = c.stream;
  const TapeLayout T = tape_layout(num_atoms, nf, H, n_layers);
  LgArgs G = lg_args(num_mols, num_atoms, max_mol_atoms, nf, c.mol_ptr, c.r_cut, c.box, nullptr, nullptr, nullptr,
                     nullptr, c.dt, c.cw, c.err_flag, base + W.lg);
  G.smap = smap;
  AuxPipe pipe(st, n_layers);
  if (!pipe.ok()) return -2;
  lg_setup(st, G);
  const int grid = lg_grid(G);
  const int ga = (num_atoms + BLOCK - 1) / BLOCK;
  for (int l = n_layers - 1; l >= 0; --l) {
    float* const wb = ws + Wl.buf0 + (size_t)(l % Wl.nbuf) * Wl.span;
    int32_t* const boff_l = boff + (size_t)(l % Wl.nbuf) * (W.nb + 1);
    int32_t* const tot_l = tot + l % Wl.nbuf;
    if (!pipe.wait_free(l, Wl.nbuf)) return -2;
    G.pos = const_cast<float*>(c.tape + T.pos + (size_t)l * num_atoms * 3);
    lg_search(st, G);
    ENFLOW_TIMED("lg_bwd_offsets_kernel", st, hipLaunchKernelGGL(lg_bwd_offsets_kernel, dim3(1), dim3(BLOCK), 0, st, c.mol_ptr, num_mols, G.blk_start, G.rbl,
                       G.npairs, boff_l, tot_l));
    BwdArgs A = layer_bwd_args(c, l, wb, Wl);
    A.blk_start = G.blk_start; A.rbl = G.rbl; A.max_n = max_mol_atoms;
    A.npairs_g = G.npairs; A.cntrow_g = G.cntrow; A.pairs_g = G.pairs;
    A.boff = boff_l; A.rowstart = rowstart; A.colc = colc; A.prb = c.pair_row_bound;
    launch_layer_bwd(H, 32, true, c.f32b, c.variants, c.ldj_atoms, grid, st, A);
    if (num_atoms > 0) {
      ENFLOW_TIMED("lg_colsum_kernel", st, hipLaunchKernelGGL(lg_colsum_kernel, dim3(ga, W.nch), dim3(BLOCK), 0, st, c.mol_ptr, num_mols, num_atoms,
                         max_mol_atoms, smap, rowstart, colc, nf, part));
      ENFLOW_TIMED("lg_colfinal_kernel", st, hipLaunchKernelGGL(lg_colfinal_kernel, dim3((num_atoms + WAVES - 1) / WAVES), dim3(BLOCK), 0, st, c.mol_ptr, num_mols, num_atoms, G.idmap,
                         part, W.nch, nf, c.adj_h, c.adj_pos));
    }
    if (!pipe.layer_queued(l)) return -2;
    const int rc = layer_weight_grads(c, l, pipe.aux(), Wl, wb, tot_l);
    if (rc) return rc;
    if (!pipe.grads_queued(l)) return -2;
  }
  if (!pipe.join()) return -2;
  if (c.kind == ENFLOW_DEQUANT_ARGMAX && num_atoms > 0) {
    const int chunks = (num_atoms + 31) / 32;
    hipLaunchKernelGGL(chunk_ptr_kernel, dim3(chunks / BLOCK + 1), dim3(BLOCK), 0, st, num_atoms, chunks, chunk);
    const int rc = argmax_grads(c, Wl, ws + Wl.buf0, chunk, chunks, 32);
    if (rc) return rc;
  }
  return poison_grads(c);
}

int enflow_lf_backward_large_f32(int num_mols, int num_atoms, int max_mol_atoms, int nf, int H,
                                 const int32_t* mol_ptr, const float* r_cut, const float* box, const float* tape,
                                 const float* layers, const float* layers_bwd, const float* layers_raw, int n_layers,
                                 int dequant_kind, const float* dequant_raw, const float* h_data, const float* noise,
                                 float dt, float cw,
                                 float* adj_h, float* adj_g, float* adj_pos, float* adj_vel, const float* adj_ldj,
                                 float* grad_layers, float* grad_dequant,
                                 void* workspace, int64_t workspace_bytes, int64_t pair_row_bound,
                                 int32_t* err_flag, void* stream) {
  BwdCall c;
  c.num_mols = num_mols; c.num_atoms = num_atoms; c.max_mol_atoms = max_mol_atoms; c.nf = nf; c.H = H;
  c.n_layers = n_layers; c.mol_ptr = mol_ptr; c.r_cut = r_cut; c.box = box; c.tape = tape;
  c.layers = layers; c.layers_bwd = layers_bwd; c.layers_raw = layers_raw; c.dt = dt; c.cw = cw;
  c.dequant_raw = dequant_raw; c.h_data = h_data; c.noise = noise; c.grad_dequant = grad_dequant;
  c.adj_h = adj_h; c.adj_g = adj_g; c.adj_pos = adj_pos; c.adj_vel = adj_vel; c.adj_ldj = adj_ldj;
  c.grad_layers = grad_layers; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
  c.pair_row_bound = pair_row_bound; c.err_flag = err_flag; c.stream = S(stream);
  decode_flags(c, dequant_kind, false);
  return lf_backward_large_impl(c);
}

// ---- standalone EGCL.forward backward ------------------------------------
// Workspace: the one-layer backward's, then scratch for the (unused) velocity /
// g adjoints and a zero log|detJ| adjoint.
static size_t egcl_bwd_extra(int num_atoms, int nf) {
  return al64((size_t)num_atoms * 3) + al64((size_t)num_atoms * nf) + 64;
}
int64_t enflow_egcl_backward_workspace_size(int num_mols, int num_atoms, int nf, int H, int64_t pair_row_bound) {
  if (num_mols < 0 || num_atoms < 0 || nf < 1 || nf > BWD_NFMAX || !hid_ok(H) || pair_row_bound < 0) return -1;
  return (int64_t)((bwd_ws(num_mols, num_atoms, nf, H, 1, pair_row_bound).total + egcl_bwd_extra(num_atoms, nf)) *
                   sizeof(float));
}

// The one-layer call of a standalone EGCL backward (dequant NONE, dt 0) with the
// extra section at `extra` carved into the unused velocity / g adjoints and the
// log|detJ| adjoint, which is zeroed on the stream; -2 if that fails.
static int egcl_call(BwdCall& c, float* extra, int egcl_flags, const float* adj_Q, const float* adj_F,
                     const float* adj_G) {
  c.n_layers = 1;
  c.adj_vel = extra;
  c.adj_g = c.adj_vel + al64((size_t)c.num_atoms * 3);
  float* zero = c.adj_g + al64((size_t)c.num_atoms * c.nf);
  c.adj_ldj = zero;
  c.eg_dQ = adj_Q; c.eg_dF = adj_F; c.eg_dG = adj_G;
  decode_flags(c, egcl_flags, true);
  return hipMemsetAsync(zero, 0, 64 * sizeof(float), c.stream) == hipSuccess ? 0 : -2;
}

int enflow_egcl_backward_f32(int num_mols, int num_atoms, int max_mol_atoms, int nf, int H,
                             const int32_t* mol_ptr, const float* r_cut, const float* box,
                             const float* tape, const int32_t* pair_counts,
                             const float* layer, const float* layer_bwd, const float* layer_raw, int egcl_flags,
                             float cw, const float* adj_Q, const float* adj_F, const float* adj_G,
                             float* adj_h, float* adj_pos, float* grad_layer,
                             void* workspace, int64_t workspace_bytes, int64_t pair_row_bound,
                             int32_t* err_flag, void* stream) {
  if (num_mols < 0 || num_atoms < 0 || nf < 1 || nf > BWD_NFMAX || !hid_ok(H) || pair_row_bound < 0) return -1;
  if (!adj_Q || !adj_F || !adj_G || !workspace) return -1;
  const BwdWs Wl = bwd_ws(num_mols, num_atoms, nf, H, 1, pair_row_bound);
  if ((uint64_t)workspace_bytes < (Wl.total + egcl_bwd_extra(num_atoms, nf)) * sizeof(float)) return -6;
  BwdCall c;
  c.num_mols = num_mols; c.num_atoms = num_atoms; c.max_mol_atoms = max_mol_atoms; c.nf = nf; c.H = H;
  c.mol_ptr = mol_ptr; c.r_cut = r_cut; c.box = box; c.tape = tape; c.pair_counts = pair_counts;
  c.layers = layer; c.layers_bwd = layer_bwd; c.layers_raw = layer_raw; c.cw = cw;
  c.adj_h = adj_h; c.adj_pos = adj_pos; c.grad_layers = grad_layer; c.workspace = workspace;
  c.workspace_bytes = workspace_bytes; c.pair_row_bound = pair_row_bound; c.err_flag = err_flag; c.stream = S(stream);
  if (egcl_call(c, reinterpret_cast<float*>(workspace) + Wl.total, egcl_flags, adj_Q, adj_F, adj_G)) return -2;
  return lf_backward_impl(c);
}

// molecules past 64 atoms: the large-system backward on a one-layer tape of
// enflow_lf_forward_large_f32 (dt 0, dequant NONE)
int64_t enflow_egcl_backward_large_workspace_size(int num_mols, int num_atoms, int max_mol_atoms, int nf, int H,
                                                  int64_t pair_row_bound) {
  const int64_t w = enflow_lf_backward_large_workspace_size(num_mols, num_atoms, max_mol_atoms, nf, H,
                                                            pair_row_bound);
  if (w < 0) return -1;
  return w + (int64_t)(egcl_bwd_extra(num_atoms, nf) * sizeof(float));
}

int enflow_egcl_backward_large_f32(int num_mols, int num_atoms, int max_mol_atoms, int nf, int H,
                                   const int32_t* mol_ptr, const float* r_cut, const float* box, const float* tape,
                                   const float* layer, const float* layer_bwd, const float* layer_raw,
                                   int egcl_flags, float cw, const float* adj_Q, const float* adj_F,
                                   const float* adj_G, float* adj_h, float* adj_pos, float* grad_layer,
                                   void* workspace, int64_t workspace_bytes, int64_t pair_row_bound,
                                   int32_t* err_flag, void* stream) {
  const int64_t w = enflow_lf_backward_large_workspace_size(num_mols, num_atoms, max_mol_atoms, nf, H,
                                                            pair_row_bound);
  if (w < 0 || !adj_Q || !adj_F || !adj_G || !workspace) return -1;
  if (workspace_bytes < w + (int64_t)(egcl_bwd_extra(num_atoms, nf) * sizeof(float))) return -6;
  BwdCall c;
  c.num_mols = num_mols; c.num_atoms = num_atoms; c.max_mol_atoms = max_mol_atoms; c.nf = nf; c.H = H;
  c.mol_ptr = mol_ptr; c.r_cut = r_cut; c.box = box; c.tape = tape;
  c.layers = layer; c.layers_bwd = layer_bwd; c.layers_raw = layer_raw; c.cw = cw;
  c.adj_h = adj_h; c.adj_pos = adj_pos; c.grad_layers = grad_layer; c.workspace = workspace;
  c.workspace_bytes = w; c.pair_row_bound = pair_row_bound; c.err_flag = err_flag; c.stream = S(stream);
  if (egcl_call(c, reinterpret_cast<float*>(static_cast<char*>(workspace) + w), egcl_flags, adj_Q, adj_F, adj_G))
    return -2;
  return lf_backward_large_impl(c);
}

// ---- LFIntegrator.reverse backward ---------------------------------------
// Host loop over the layers in the order opposite to the reverse pass's (layer
// 0 ran last).  Per layer: the one-layer tape at the taped post-layer (h', x')
// exactly as the standalone EGCL backward is fed (a one-layer forward, dequant
// NONE, dt 0), lf_rev_adj_pre, the standalone EGCL backward (fused up to 64
// atoms per molecule, large-system past that) with its weight gradients into the
// layer's slice of grad_layers, lf_rev_adj_post.
struct RevBwdWs {
  size_t hw, gw, pw, vw, ldj_mol, ldj, counts, aQ, aF, aG, dh, dx, tape, lg, eg, total;
  int64_t lg_bytes, eg_bytes;
  bool large;
};
static int rev_bwd_ws(int num_mols, int num_atoms, int max_n, int nf, int H, int64_t prb, RevBwdWs& W) {
  if (num_mols < 0 || num_atoms < 0 || max_n < 0 || max_n >= (1 << 22) || nf < 1 || nf > BWD_NFMAX || !hid_ok(H) ||
      prb < 0 || prb > 0x7fffffffLL)
    return -1;
  W.large = max_n > 64;
  const int64_t tape = enflow_lf_tape_size_for(num_atoms, nf, H, 1, max_n);
  W.lg_bytes = W.large ? enflow_lf_large_workspace_size(num_mols, num_atoms, max_n, nf) : 0;
  W.eg_bytes = W.large ? enflow_egcl_backward_large_workspace_size(num_mols, num_atoms, max_n, nf, H, prb)
                       : enflow_egcl_backward_workspace_size(num_mols, num_atoms, nf, H, prb);
  if (tape < 0 || W.lg_bytes < 0 || W.eg_bytes < 0) return -1;
  const size_t A = (size_t)num_atoms, f = sizeof(float);
  size_t o = 0;
  W.hw = o; o = al256(o + A * nf * f);
  W.gw = o; o = al256(o + A * nf * f);
  W.pw = o; o = al256(o + A * 3 * f);
  W.vw = o; o = al256(o + A * 3 * f);
  W.ldj_mol = o; o = al256(o + ((size_t)num_mols + 1) * f);
  W.ldj = o; o = al256(o + f);
  W.counts = o; o = al256(o + ((size_t)num_mols + 1) * sizeof(int32_t));
  W.aQ = o; o = al256(o + A * f);
  W.aF = o; o = al256(o + A * 3 * f);
  W.aG = o; o = al256(o + A * nf * f);
  W.dh = o; o = al256(o + A * nf * f);
  W.dx = o; o = al256(o + A * 3 * f);
  W.tape = o; o = al256(o + (size_t)tape * f);
  W.lg = o; o = al256(o + (size_t)W.lg_bytes);
  W.eg = o; o = al256(o + (size_t)W.eg_bytes);
  W.total = o;
  return 0;
}

int64_t enflow_lf_reverse_backward_workspace_size(int num_mols, int num_atoms, int max_mol_atoms, int nf, int H,
                                                  int64_t pair_row_bound) {
  RevBwdWs W;
  if (rev_bwd_ws(num_mols, num_atoms, max_mol_atoms, nf, H, pair_row_bound, W)) return -1;
  return (int64_t)W.total;
}

int enflow_lf_reverse_backward_f32(int num_mols, int num_atoms, int max_mol_atoms, int nf, int H,
                                   const int32_t* mol_ptr, const float* r_cut, const float* box,
                                   const float* state_h, const float* state_pos, const float* state_vel,
                                   const float* layers, const float* layers_bwd, const float* layers_raw,
                                   int n_layers, int flags, int gemm_precision, float dt, float cw,
                                   float* adj_h, float* adj_g, float* adj_pos, float* adj_vel,
                                   const float* adj_ldj, float* grad_layers,
                                   void* workspace, int64_t workspace_bytes, int64_t pair_row_bound,
                                   int32_t* err_flag, void* stream) {
  RevBwdWs W;
  if (rev_bwd_ws(num_mols, num_atoms, max_mol_atoms, nf, H, pair_row_bound, W) || n_layers < 0) return -1;
  const int gp = gemm_precision & 0xff;
  if (gp != ENFLOW_PREC_F32 && gp != ENFLOW_PREC_F16X3) return -1;
  if (!mol_ptr || !r_cut || !box || !state_h || !state_pos || !state_vel || !layers || !layers_bwd || !layers_raw ||
      !adj_h || !adj_g || !adj_pos || !adj_vel || !adj_ldj || !grad_layers || !workspace || !err_flag)
    return -1;
  if ((uint64_t)workspace_bytes < W.total) return -6;
  if (num_mols == 0 || num_atoms == 0 || n_layers == 0) return 0;
  hipStream_t st = S(stream);
  char* base = static_cast<char*>(workspace);
  auto fp = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
  float *hw = fp(W.hw), *gw = fp(W.gw), *pw = fp(W.pw), *vw = fp(W.vw), *tape = fp(W.tape);
  float *aQ = fp(W.aQ), *aF = fp(W.aF), *aG = fp(W.aG), *dh = fp(W.dh), *dx = fp(W.dx);
  int32_t* counts = reinterpret_cast<int32_t*>(base + W.counts);
  // the tape of an fp32-GEMM forward gets the fp32 backward
  const int eg_flags = ((flags & ENFLOW_EGCL_VARIANTS) ? 1 : 0) |
                       ((flags & ENFLOW_BWD_F32) || gp == ENFLOW_PREC_F32 ? ENFLOW_BWD_F32 : 0);
  const size_t A = (size_t)num_atoms;
  const RawEgcl R = raw_egcl(H, nf);
  const float* Q = tape + tape_layout(num_atoms, nf, H, 1).q;
  const int ga = cdiv(num_atoms, BLOCK);
  for (int l = 0; l < n_layers; ++l) {
    const float* Lp = layers + (size_t)l * egcl_layout(H, nf).total;
    const float* Bp = layers_bwd + (size_t)l * egcl_bwd_layout(H).total;
    const float* Rp = layers_raw + (size_t)l * R.total_bwd;
    if (hipMemcpyAsync(hw, state_h + (size_t)l * A * nf, A * nf * sizeof(float), hipMemcpyDeviceToDevice, st) !=
            hipSuccess ||
        hipMemcpyAsync(pw, state_pos + (size_t)l * A * 3, A * 3 * sizeof(float), hipMemcpyDeviceToDevice, st) !=
            hipSuccess ||
        hipMemsetAsync(gw, 0, A * nf * sizeof(float), st) != hipSuccess ||
        hipMemsetAsync(vw, 0, A * 3 * sizeof(float), st) != hipSuccess ||
        hipMemsetAsync(counts, 0, ((size_t)num_mols + 1) * sizeof(int32_t), st) != hipSuccess)
      return -2;
    int rc;
    if (W.large)
      rc = enflow_lf_forward_large_f32(num_mols, num_atoms, max_mol_atoms, nf, H, mol_ptr, r_cut, box, hw, gw, pw, vw,
                                       Lp, 1, ENFLOW_DEQUANT_NONE, nullptr, nullptr, 0.f, 0.f, cw, fp(W.ldj_mol),
                                       fp(W.ldj), err_flag, gemm_precision, tape, counts, base + W.lg, W.lg_bytes,
                                       stream);
    else
      rc = enflow_lf_forward_f32(num_mols, num_atoms, max_mol_atoms, nf, H, mol_ptr, r_cut, box, hw, gw, pw, vw, Lp,
                                 1, ENFLOW_DEQUANT_NONE, nullptr, nullptr, 0.f, 0.f, cw, fp(W.ldj_mol), fp(W.ldj),
                                 err_flag, nullptr, tape, counts, gemm_precision, stream);
    if (rc) return rc;
    ENFLOW_TIMED("lf_rev_adj_pre", st,
                 hipLaunchKernelGGL(lf_rev_adj_pre, dim3(ga), dim3(BLOCK), 0, st, mol_ptr, num_mols, num_atoms, nf, dt,
                                    state_vel + (size_t)l * A * 3, Q, adj_g, adj_vel, adj_ldj, aQ, aF, aG));
    float* grad = grad_layers + (size_t)l * R.total_bwd;
    if (W.large)
      rc = enflow_egcl_backward_large_f32(num_mols, num_atoms, max_mol_atoms, nf, H, mol_ptr, r_cut, box, tape, Lp, Bp,
                                          Rp, eg_flags, cw, aQ, aF, aG, dh, dx, grad, base + W.eg, W.eg_bytes,
                                          pair_row_bound, err_flag, stream);
    else
      rc = enflow_egcl_backward_f32(num_mols, num_atoms, max_mol_atoms, nf, H, mol_ptr, r_cut, box, tape, counts, Lp,
                                    Bp, Rp, eg_flags, cw, aQ, aF, aG, dh, dx, grad, base + W.eg, W.eg_bytes,
                                    pair_row_bound, err_flag, stream);
    if (rc) return rc;
    ENFLOW_TIMED("lf_rev_adj_post", st,
                 hipLaunchKernelGGL(lf_rev_adj_post, dim3(ga), dim3(BLOCK), 0, st, num_atoms, nf, dt, Q, dh, dx, adj_h,
                                    adj_g, adj_pos, adj_vel));
  }
  BwdCall c;   // no dequantiser: the layers' gradients alone
  c.nf = nf; c.H = H; c.n_layers = n_layers; c.grad_layers = grad_layers; c.err_flag = err_flag; c.stream = st;
  return poison_grads(c);
}

// ---- EGCL.forward backward on a caller-supplied edge list -------------------
// el_bwd_offsets_kernel, lf_layer_bwd_kernel<.., BIG, LIST> per block of 32 rows
// of the CSR (row-side d h in LDS, d coord_diff per edge, column-side d h per edge
// into colc), el_colsum_kernel over the host's CSC view, then the weight
// gradients on the auxiliary stream as everywhere else.  The instances
// LAYER_BWD_BIG has, named after it in the code object.
static void launch_layer_bwd_list(int H, bool f32b, bool variants, int grid, hipStream_t st, const BwdArgs& A) {
#define LAYER_BWD_LIST(HH, VARF, PRECF)                                                                   \
  ENFLOW_TIMED("lf_layer_bwd_kernel_list", st,                                                           \
               hipLaunchKernelGGL((lf_layer_bwd_kernel<HH, 32, VARF, PRECF, true, true>), dim3(grid), dim3(BLOCK), 0, st, A))
#define LAYER_BWD_LIST_H(HH)                                        \
  do {                                                              \
    if (f32b) LAYER_BWD_LIST(HH, true, PREC_F32);                   \
    else if (variants) LAYER_BWD_LIST(HH, true, PREC_F16X3);        \
    else LAYER_BWD_LIST(HH, false, PREC_F16X3);                     \
  } while (0)
  DISPATCH_H(H, LAYER_BWD_LIST_H);
#undef LAYER_BWD_LIST_H
#undef LAYER_BWD_LIST
}

// pair rows: every block of 32 rows rounds its edges up to a tile
static inline long long el_pair_row_bound(int num_nodes, int64_t num_edges) {
  return (long long)num_edges + 31LL * ((num_nodes + 31) / 32);
}
struct ElBwdWs { size_t bwd, colc, boff, tot, total; };
static ElBwdWs el_bwd_ws(int num_nodes, int64_t num_edges, int nf, int H) {
  ElBwdWs W;
  size_t o = 0;
  // one buffer of pair / node rows (a single layer: nothing to rotate)
  const BwdWs Wl = bwd_ws(1, num_nodes, nf, H, 0, el_pair_row_bound(num_nodes, num_edges));
  W.bwd = o; o = al256(o + (Wl.buf0 + Wl.span) * sizeof(float));
  W.colc = o; o = al256(o + (size_t)num_edges * CSTR * 4);
  W.boff = o; o = al256(o + ((size_t)(num_nodes + 31) / 32 + 1) * 4);
  W.tot = o; o = al256(o + 4);
  W.total = o;
  return W;
}
// the limits of enflow_egcl_forward_list_f32, and int32 pair rows
static int el_limits(int num_nodes, int64_t num_edges, int nf, int H) {
  if (num_nodes < 0 || num_edges < 0) return -1;
  if (nf < 1 || nf > BWD_NFMAX) return -4;
  if (!hid_ok(H)) return -5;
  if (num_nodes > (1 << 22) || num_edges > (int64_t)INT32_MAX - 1024 ||
      el_pair_row_bound(num_nodes, num_edges) > 0x7fffffffLL)
    return -3;
  return 0;
}

int64_t enflow_egcl_backward_list_workspace_size(int num_nodes, int64_t num_edges, int nf, int H) {
  const int rc = el_limits(num_nodes, num_edges, nf, H);
  if (rc) return rc;
  return (int64_t)el_bwd_ws(num_nodes, num_edges, nf, H).total;
}

int enflow_egcl_backward_list_f32(int num_nodes, int64_t num_edges, int nf, int H,
                                  const int32_t* row_ptr, const int32_t* col, const float* coord_diff,
                                  const int32_t* col_ptr, const int32_t* col_perm, const float* tape,
                                  const float* layer, const float* layer_bwd, const float* layer_raw,
                                  int egcl_flags, float cw, const float* adj_Q, const float* adj_F,
                                  const float* adj_G, float* adj_h, float* adj_coord_diff, float* grad_layer,
                                  void* workspace, int64_t workspace_bytes, int32_t* err_flag, void* stream) {
  const int lim = el_limits(num_nodes, num_edges, nf, H);
  if (lim) return lim;
  if (egcl_flags & ~(0xff | ENFLOW_BWD_F32)) return -1;
  if (!row_ptr || !col_ptr || !tape || !layer || !layer_bwd || !layer_raw || !adj_Q || !adj_F || !adj_G || !adj_h ||
      !grad_layer || !workspace || !err_flag ||
      (num_edges > 0 && (!col || !coord_diff || !col_perm || !adj_coord_diff)))
    return -1;
  const ElBwdWs W = el_bwd_ws(num_nodes, num_edges, nf, H);
  if (workspace_bytes < 0 || (uint64_t)workspace_bytes < W.total) return -6;
  if (num_nodes == 0) return 0;
  const long long prb = el_pair_row_bound(num_nodes, num_edges);
  const BwdWs Wl = bwd_ws(1, num_nodes, nf, H, 0, prb);
  char* base = static_cast<char*>(workspace);
  float* wb = reinterpret_cast<float*>(base + W.bwd) + Wl.buf0;
  float* colc = reinterpret_cast<float*>(base + W.colc);
  int32_t* boff = reinterpret_cast<int32_t*>(base + W.boff);
  int32_t* tot = reinterpret_cast<int32_t*>(base + W.tot);
  // the one-layer case: the nodes are one "molecule" without a batch, only d h is an adjoint
  BwdCall c;
  c.num_mols = 1; c.num_atoms = num_nodes; c.nf = nf; c.H = H; c.n_layers = 1; c.tape = tape;
  c.layers = layer; c.layers_bwd = layer_bwd; c.layers_raw = layer_raw; c.cw = cw; c.adj_h = adj_h;
  c.grad_layers = grad_layer; c.pair_row_bound = prb; c.err_flag = err_flag; c.stream = S(stream);
  c.eg_dQ = adj_Q; c.eg_dF = adj_F; c.eg_dG = adj_G;
  decode_flags(c, egcl_flags, true);
  hipStream_t st = c.stream;
  AuxPipe pipe(st, 1);
  if (!pipe.ok()) return -2;
  const int grid = (num_nodes + 31) / 32;
  ENFLOW_TIMED("el_bwd_offsets_kernel", st, hipLaunchKernelGGL(el_bwd_offsets_kernel, dim3(1), dim3(BLOCK), 0, st, row_ptr, num_nodes, (int)num_edges, prb,
                     boff, tot, err_flag));
  BwdArgs A = layer_bwd_args(c, 0, wb, Wl);
  A.boff = boff; A.colc = colc; A.prb = prb;
  A.l_row_ptr = row_ptr; A.l_col = col; A.l_cdiff = coord_diff; A.l_acd = adj_coord_diff;
  A.l_edges = (int)num_edges;
  launch_layer_bwd_list(H, c.f32b, c.variants, grid, st, A);
  if (num_edges > 0)
    ENFLOW_TIMED("el_colsum_kernel", st, hipLaunchKernelGGL(el_colsum_kernel, dim3((num_nodes + WAVES - 1) / WAVES), dim3(BLOCK), 0, st, col_ptr, col_perm,
                       num_nodes, (int)num_edges, colc, nf, adj_h, err_flag));
  if (!pipe.layer_queued(0)) return -2;
  const int rc = layer_weight_grads(c, 0, pipe.aux(), Wl, wb, tot);
  if (rc) return rc;
  if (!pipe.grads_queued(0) || !pipe.join()) return -2;
  // a set error word leaves NaN in every gradient, d h and d coord_diff included
  hipLaunchKernelGGL(poison_on_err_kernel, dim3(64), dim3(256), 0, st, err_flag, grad_layer,
                     (long long)raw_egcl(H, nf).total_bwd, adj_h, (long long)num_nodes * nf);
  if (num_edges > 0)
    hipLaunchKernelGGL(poison_on_err_kernel, dim3(64), dim3(256), 0, st, err_flag, adj_coord_diff,
                       (long long)num_edges * 3, nullptr, 0LL);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// ---- standalone ArgMax.forward backward ------------------------------------
struct AmBwdWs { size_t apre, spre, anet, part, total; };
static AmBwdWs am_bwd_ws(int num_atoms, int nf, int H) {
  AmBwdWs W;
  size_t o = 0;
  const size_t A = (size_t)num_atoms;
  W.apre = o; o += al64(A * H);
  W.spre = o; o += al64(A * H);
  W.anet = o; o += al64(A * 2 * nf);
  const size_t cha = (size_t)cdiv(num_atoms, OA_CHUNK_ATOM);
  W.part = o; o += al64(cha * ((size_t)H * (nf + 1) + (size_t)2 * nf * (H + 1)));
  W.total = o;
  return W;
}
int64_t enflow_argmax_backward_workspace_size(int num_atoms, int nf, int H) {
  if (num_atoms < 0 || nf < 1 || nf > NFMAX || !hid_ok(H)) return -1;
  return (int64_t)(am_bwd_ws(num_atoms, nf, H).total * sizeof(float));
}

int enflow_argmax_backward_f32(int num_mols, int num_atoms, int max_mol_atoms, int nf, int H,
                               const int32_t* mol_ptr, const float* h, const float* dequant_raw, const float* noise,
                               const float* adj_z, const float* adj_log_q, float* grad_dequant,
                               void* workspace, int64_t workspace_bytes, void* stream) {
  if (num_mols < 0 || num_atoms < 0 || max_mol_atoms < 0 || max_mol_atoms > 64 || nf < 1 || nf > BWD_NFMAX ||
      !hid_ok(H))
    return -1;
  if (!mol_ptr || !h || !dequant_raw || !noise || !adj_z || !adj_log_q || !grad_dequant || !workspace) return -1;
  const AmBwdWs W = am_bwd_ws(num_atoms, nf, H);
  if ((uint64_t)workspace_bytes < W.total * sizeof(float)) return -6;
  if (num_mols == 0) return 0;
  hipStream_t st = S(stream);
  float* ws = reinterpret_cast<float*>(workspace);
  float *apre = ws + W.apre, *spre = ws + W.spre, *anet = ws + W.anet;
  argmax_bwd_launch(H, max_mol_atoms, num_mols, st, mol_ptr, nf, h, noise, dequant_raw, adj_z, adj_log_q, apre, spre, anet);
  const int rW1 = 0, rb1 = H * nf, rW2 = rb1 + H, rb2 = rW2 + 2 * nf * H;
  OuterBatch ob;
  ob.nd = 0;
  float* part = ws + W.part;
  add_desc(ob, apre, H, H, h, nf, nf, nullptr, num_atoms, num_atoms, part, grad_dequant + rW1,
           grad_dequant + rb1);
  add_desc(ob, anet, 2 * nf, 2 * nf, spre, H, H, nullptr, num_atoms, num_atoms, part, grad_dequant + rW2,
           grad_dequant + rb2);
  return run_outer(ob, st);
}

}  // extern "C"
