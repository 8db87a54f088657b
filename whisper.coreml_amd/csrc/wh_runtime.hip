// libwhisper_hip runtime: context, weights, buffers, stage drivers and the C ABI
// declared in include/whisper_hip.h.  The reference counterpart is the
// Objective-C++ CoreML runner coreml/coreml.mm:18-463 (process-global state, one
// model per process, void returns); here everything lives in a context object,
// every entry point returns a status, and all stage data stays in HBM.
// The audio front end (wh_audio.hip) and the host side of the decode loop and of alignment
// (wh_loop.hip) do not depend on the element type: compiled once, outside Ctx<T>.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "whisper_hip.h"
#include "wh_align.h"
#include "wh_audio.h"
#include "wh_gemm.h"
#include "wh_gemm8.h"
#include "wh_host.h"
#include "wh_kernels.h"
#include "wh_layout.h"
#include "wh_loop.h"
#include "wh_proj8.h"
#include "wh_vocab8.h"

using namespace wh;

static thread_local std::string g_release_error;  // a failed release in the last context destroy

namespace {

// encoder windows per pass (WHISPER_HIP_ENC_CHUNK overrides; activations scale with it)
static int enc_chunk() {
  static const int v = [] {
    const char* e = tune_env("WHISPER_HIP_ENC_CHUNK");
    const int c = e ? atoi(e) : 16;
    return c >= 1 && c <= 64 ? c : 16;
  }();
  return v;
}
}  // namespace

struct wh_ctx : DecodeLoop {
  virtual std::string step_kernels(int n_win, int group) const = 0;
  virtual ~wh_ctx() {}
  virtual int load(const std::string& name, const float* data, const int64_t* shape, int ndim) = 0;
  virtual int finalize() = 0;
  virtual int encode(int n_win, const int64_t* seeks, const int* segs) = 0;
  virtual int read_xa(int slot, float* out) = 0;
  virtual int read_ckv(int slot, int layer, float* k, float* v) = 0;
  virtual int set_ckv_format(int fmt) = 0;
  virtual int read_ckv8(int slot, int layer, uint8_t* kc, float* ks, uint8_t* vc, float* vs) = 0;
  virtual int set_enc_format(int fmt) = 0;
  virtual int set_dec_format(int fmt) = 0;
  virtual int read_dec_w8(int layer, int which, uint8_t* codes, float* scales) = 0;
  virtual int set_vocab_format(int fmt) = 0;
  virtual int read_vocab_w8(uint8_t* codes, float* scales) = 0;
  virtual std::string encoder_kernels(int n_win) const = 0;
  virtual int fp8_linear(int M, int N, int K, const float* x, const float* w, const float* bias, int gelu, int tile,
                         float* y, uint8_t* xc, float* xs, uint8_t* wc, float* ws) = 0;
  virtual int decode_begin(int n_win, const wh_decode_opts* o, const int* init, const int* n_init, int max_init,
                           const int* sot_index, const int* slots) = 0;
  virtual int step_prefill(int n_win, int G, const int* init, const int* n_init, int max_init, const int* sot_index,
                           float* lg) = 0;
  virtual int step_tokens(const int* tok, const int* offsets, float* lg) = 0;
  virtual int prefill_logits(int slot, const int* tokens, int n, float* logits, const int* ah, int na, float* aqk) = 0;
  virtual int time_stage(int what, int iters, double* ms) = 0;
  // tuning builds only (wh_tune_share_weights): read the weights of another context of the
  // same dims and dtype instead of this one's (probes of two window groups, one weight copy)
  virtual int share_weights_from(wh_ctx* src) = 0;
  // weight sharing (tuning builds): the contexts reading this one's weights, and the
  // context this one reads from; wh_destroy refuses a context others still read from
  int sharers = 0;
  wh_ctx* shares_from = nullptr;
  AudioFront audio;  // waveforms and the log-mel (csrc/wh_audio.h)
  int n_mels = 0;    // the model's
  int maxc_stride = 1;
  int device = 0;
};

namespace {

template <typename T>
struct Ctx : public wh_ctx {
  using elem = T;
  wh_dims d;
  int ns, La, K1p;
  LayoutDims ld;            // what the two layouts and the tensor shapes are sized by
  void* wbase = nullptr;    // weights (layout_weights)
  void* abase = nullptr;    // activations / state (layout_buffers)
  std::set<std::string> loaded;

  // weights
  T *conv1_w, *conv2_w, *E, *Pdec, *ckv_w;
  float *conv1_b, *conv2_b, *pos_enc, *lnp_g, *lnp_b, *ln_g, *ln_b, *ckv_b;
  std::vector<EncLayer<T>> enc;
  std::vector<DecLayer<T>> dec;

  std::vector<int64_t> h_seeks;

  // encoder buffers
  T *melT, *h1, *xn_e, *qkv_e, *vt_e, *att_e, *hm_e, *xa, *ckv;
  // the 8-bit copy of the cross-KV the step's cross-attention reads (wh_set_cross_kv_format:
  // [layer][slot][head][tile] records, wh_kernels.h CKV8_REC), written by k_ckv_quant behind
  // every cross-KV GEMM; null = the step reads ckv.  Allocated once, when the format is chosen
  char* ckv8 = nullptr;
  bool encoded = false;  // an encode has run: the format is fixed
  // encoder format (wh_set_encoder_format).  The 8-bit weight copies and the activation
  // codes + row scales of one GEMM input ([WE x 1500][<= 4n] bytes) are allocated when
  // WH_ENC_FP8_E4M3 is first chosen and kept until the context is destroyed
  int enc_fmt = WH_ENC_NATIVE;
  char* e8_base = nullptr;
  std::vector<Enc8Layer> enc8;
  uint8_t* e8x = nullptr;
  float* e8s = nullptr;
  bool e8_quantised = false;
  // decoder format (wh_set_decoder_format).  The 8-bit copies of the six linear weights of
  // every layer (wh_layout.h layout_dec8) are allocated when WH_DEC_FP8_E4M3 is first chosen
  // and kept until the context is destroyed; w8_step: the format the current batch began with
  int dec_fmt = WH_DEC_NATIVE;
  char* d8_base = nullptr;
  std::vector<Dec8Layer> dec8;
  bool d8_quantised = false, w8_step = false;
  // vocabulary format (wh_set_vocab_format).  The 8-bit copy of the token embedding
  // (wh_vocab8.h: v8_cols(V) x ns codes, then v8_cols(V) scales) is allocated when
  // WH_VOCAB_FP8_E4M3 is first chosen and kept until the context is destroyed; v8_step: the
  // format the current batch began with
  int vocab_fmt = WH_VOCAB_NATIVE;
  uint8_t* v8_codes = nullptr;
  float* v8_scales = nullptr;
  bool v8_quantised = false, v8_step = false;
  const void* kv8_layer(int l) const { return ckv8 ? ckv8 + (size_t)l * Wcap * ckv8_slot_bytes(nh) : nullptr; }
  float* x_e;
  int64_t* d_seeks;
  int* d_segs;
  // self KV per layer
  std::vector<T*> kc, vc;
  // decoder buffers
  int RD;
  float *x_d, *po, *pm, *pl, *logits, *logits2, *part;
  T *xn_d, *q_d, *att_d, *hm_d;
  int *row_tok, *row_pos, *row_win, *row_slot, *win_row0, *win_nrows, *win_slot, *rows_in;
  int *st_row_win, *st_row_slot, *st_win_row0, *st_win_nrows, *st_win_slot;
  int* fp_anc = nullptr;
  float* p1_slab = nullptr;  // k_proj1 in-launch split-K slabs [zs][N/16][256]
  int* p1_cnt = nullptr;     // and arrival counters [4n/16] (zero between launches)
  // single-window encoder: the residual GEMMs' K halves (k_gemm_tile KZ = 2) meet through
  // these fp32 slabs (64 KB per 128 x 64 tile, 12 x n/64 tiles at 1500 rows) and
  // per-(tile, wave) arrival counters (zero between launches)
  float* ekz_slab = nullptr;
  int* ekz_cnt = nullptr;
  float* xs_rec = nullptr;   // step cross-attention segment records [pair][XS_NSP][XREC]
  float* x2_d = nullptr;     // k_proj1 path: second residual buffer (deferred residual ping-pong)
  int* xs_cnt = nullptr;     // and (window, head) arrival counters

  // the step cross-attention's query / split arguments
  XQPart step_xq(int rows_per_window) const {
    XQPart xq;
    xq.max_rows = rows_per_window;
    xq.split_rec = xs_rec;
    xq.split_cnt = xs_cnt;
    xq.max_pairs = Wcap * nh;
    return xq;
  }
  std::vector<hipEvent_t> proj_ev;  // time_stage(7) event pairs, empty otherwise
  int proj_ev_n = 0;

  int share_weights_from(wh_ctx* src_) override {
    auto* src = dynamic_cast<Ctx<T>*>(src_);
    if (!src || src->ns != ns || src->Ld != Ld || src->La != La || src->V != V || !src->finalized)
      return fail(-2, "share_weights: a finalized context of the same dims and dtype is needed");
    conv1_w = src->conv1_w; conv2_w = src->conv2_w; E = src->E; Pdec = src->Pdec; ckv_w = src->ckv_w;
    conv1_b = src->conv1_b; conv2_b = src->conv2_b; pos_enc = src->pos_enc; lnp_g = src->lnp_g; lnp_b = src->lnp_b;
    ln_g = src->ln_g; ln_b = src->ln_b; ckv_b = src->ckv_b;
    enc = src->enc;
    dec = src->dec;
    finalized = true;
    if (shares_from) --shares_from->sharers;
    shares_from = src;
    ++src->sharers;  // src's weight arena must outlive this context (wh_destroy checks)
    // this context's 8-bit decoder copies are of the weights it reads now
    d8_quantised = false;
    if (dec_fmt == WH_DEC_FP8_E4M3 || w8_step) TRY(quantise_dec8());
    v8_quantised = false;
    if (vocab_fmt == WH_VOCAB_FP8_E4M3 || v8_step) TRY(quantise_vocab8());
    return 0;
  }

  // every release checked: the first failure is kept (rel.first) and reported by
  // wh_destroy instead of staying pending for the next context's first call
  Releases rel;
  ~Ctx() override {
    if (st) rel(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (gexec) rel(hipGraphExecDestroy(gexec), "hipGraphExecDestroy");
    if (graph) rel(hipGraphDestroy(graph), "hipGraphDestroy");
    if (st) rel(hipStreamDestroy(st), "hipStreamDestroy");
    if (wbase) rel(hipFree(wbase), "hipFree(weights)");
    if (abase) rel(hipFree(abase), "hipFree(activations)");
    if (ckv8) rel(hipFree(ckv8), "hipFree(cross-KV 8-bit copy)");
    if (e8_base) rel(hipFree(e8_base), "hipFree(encoder 8-bit copy)");
    if (d8_base) rel(hipFree(d8_base), "hipFree(decoder 8-bit copy)");
    if (v8_codes) rel(hipFree(v8_codes), "hipFree(vocabulary 8-bit copy)");
    audio.release(rel);
    scratch.release(rel, "hipFree(scratch)");
    if (h_done) rel(hipHostFree(h_done), "hipHostFree(done flags)");
    for (auto& e : poll_ev)
      if (e) rel(hipEventDestroy(e), "hipEventDestroy(poll)");
    tm.release(rel);
    (void)hipGetLastError();  // what failed above is in rel.first, not left pending
    if (!rel.first.empty()) g_release_error = rel.first;
  }

  // every weight, and every activation / state buffer, named once (csrc/wh_layout.h)
  void layout_weights(Arena& ar) { wh::layout_weights(*this, ar, ld); }
  void layout_buffers(Arena& ar) { wh::layout_buffers(*this, ar, ld); }
  // One device allocation for what `layout` takes: a run on a measuring arena gives the
  // size, the allocation is that plus ARENA_TAIL_PAD, a second run carves it
  template <class F>
  int carve(void** base, Arena& ar, F layout, const char* what) {
    Arena m;
    layout(m);
    HIPCHK(hipMalloc(base, m.off + ARENA_TAIL_PAD));
    ar = Arena(*base, m.off + ARENA_TAIL_PAD);
    layout(ar);
    if (!ar.ok() || ar.off != m.off) return fail(-3, std::string(what) + " arena overflow");
    return 0;
  }

  int init(int device_, const wh_dims& dims, int Wcap_, int Gcap_) {
    device = device_;
    d = dims;
    ns = d.n_text_state;
    nh = d.n_text_head;
    La = d.n_audio_layer;
    Ld = d.n_text_layer;
    V = d.n_vocab;
    n_mels = d.n_mels;
    if (d.n_audio_state != ns || d.n_audio_head != nh) return fail(-2, "audio/text state or head mismatch unsupported");
    if (ns != nh * 64) return fail(-2, "head dim must be 64 (decoder.py:62-64)");
    if (d.n_audio_ctx != 1500 || d.n_text_ctx != CTX) return fail(-2, "n_audio_ctx must be 1500, n_text_ctx 448");
    if (ns % 128 || ns > 2048) return fail(-2, "n_state must be a multiple of 128 and <= 2048");
    if (V > 57344) return fail(-2, "n_vocab too large");
    Wcap = Wcap_;
    Gcap = Gcap_;
    if (Wcap < 1 || Gcap < 1 || Gcap > 8) return fail(-2, "bad max_windows / max_group");
    const int kb = 128 / (int)sizeof(T);
    K1p = ((3 * n_mels + kb - 1) / kb) * kb;
    HIPCHK(hipSetDevice(device));
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    TRY(tm.create());
    HIPCHK(hipHostMalloc((void**)&h_done, sizeof(int) * 2 * Wcap));  // two poll buffers
    for (auto& e : poll_ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    // the self-attention kernels address one layer's self-K / V cache with 32-bit byte
    // offsets (buffer loads, wh_kernels.hip k_self_attn / k_self_attn_qkv)
    if ((int64_t)Wcap * Gcap * CTX * ns * (int64_t)sizeof(T) >= ((int64_t)1 << 31) - 4096)
      return fail(-3, "self-KV cache of one layer exceeds 2 GiB: lower max_windows or max_group");
    // first-pass rows per pass: every window's word-timestamp alignment (<= ~230 tokens)
    // fits one pass, so its GEMMs run at M in the thousands
    PRE = std::max(PRE_ROWS, std::min(Wcap * 240, 8192));
    RD = std::max(Wcap * Gcap, PRE);
    ld = LayoutDims{(size_t)ns, (size_t)n_mels, (size_t)K1p, (size_t)La, (size_t)Ld, (size_t)V, (size_t)nh,
                    (size_t)Wcap, (size_t)Gcap, (size_t)std::min(Wcap, enc_chunk()), (size_t)RD,
                    (size_t)std::max(Wcap * Gcap, 2 * Wcap), xattn_fused_q(ns, 1, (int)sizeof(T)),
                    TKP, CTX, HCTX, LP_SLICES * LP_REC, XS_NSP * XREC, BIAS_MAX_ENTRIES};
    // both arenas start zeroed: the arrival counters and the padding keys depend on it
    Arena wa, aa;
    TRY(carve(&wbase, wa, [&](Arena& ar) { layout_weights(ar); }, "weight"));
    HIPCHK(hipMemset(wbase, 0, wa.cap));
    TRY(carve(&abase, aa, [&](Arena& ar) { layout_buffers(ar); }, "activation"));
    HIPCHK(hipMemset(abase, 0, aa.cap));
    S.nw = Wcap; S.G = 1; S.ctx = CTX; S.hctx = HCTX; S.maxc = 16;
    return audio.init(st, stats);
  }

  // ------------------------------------------------------------ weights
  // (U)(src * scale), the product in fp32 (times 1 is the value itself)
  template <typename U>
  int upload(U* dst, const float* src, size_t cnt, float scale = 1.f) {
    std::vector<U> t(cnt);
    for (size_t i = 0; i < cnt; ++i) t[i] = (U)(src[i] * scale);
    HIPCHK(hipMemcpy(dst, t.data(), cnt * sizeof(U), hipMemcpyHostToDevice));
    return 0;
  }
  // a convolution weight [n][cin][3] -> tap-major rows [o][j * cin + c] of ld >= 3 * cin elements
  int upload_conv(T* dst, const float* w, size_t cin, size_t ld) {
    std::vector<float> t(ns * ld, 0.f);
    for (size_t o = 0; o < (size_t)ns; ++o)
      for (size_t c = 0; c < cin; ++c)
        for (int j = 0; j < 3; ++j) t[o * ld + j * cin + c] = w[(o * cin + c) * 3 + j];
    return upload(dst, t.data(), t.size());
  }
  // tab's row `key` into obj (-1: no such row): the one shape check, then the upload
  template <class O, class L>
  int load_row(O& obj, const std::vector<Tensor<L, T>>& tab, const char* key, bool dec_layer, const std::string& name,
               const float* data, const int64_t* shape, int ndim) {
    for (const auto& r : tab) {
      if (strcmp(r.name, key)) continue;
      if ((int)strlen(r.shape) != ndim) return fail(-4, name + ": bad rank");
      size_t cnt = 1;
      for (int i = 0; i < ndim; ++i) {
        if (shape[i] != dim_size(r.shape[i], ld)) return fail(-4, name + ": bad shape");
        cnt *= shape[i];
      }
      if (!r.wt) return upload(obj.*(r.wf) + r.slot * cnt, data, cnt, r.scale[dec_layer]);
      T* dst = obj.*(r.wt) + r.slot * cnt;
      if (dst == conv1_w) return upload_conv(dst, data, n_mels, K1p);
      if (dst == conv2_w) return upload_conv(dst, data, ns, 3 * (size_t)ns);
      return upload(dst, data, cnt, r.scale[dec_layer]);
    }
    return -1;
  }

  int load(const std::string& name, const float* data, const int64_t* shape, int ndim) override {
    if (sharers > 0 || shares_from) return fail(-9, "load " + name + ": this context's weights are shared with another");
    int l = -1, rc;
    char part[128];
    const bool is_enc = sscanf(name.c_str(), "encoder.blocks.%d.%127s", &l, part) == 2;
    const bool is_dec = !is_enc && sscanf(name.c_str(), "decoder.blocks.%d.%127s", &l, part) == 2;
    if ((is_enc || is_dec) && (l < 0 || l >= (is_enc ? La : Ld))) return fail(-5, "layer out of range " + name);
    if (is_enc) rc = load_row(enc[l], block_tensors<T>(), part, false, name, data, shape, ndim);
    else if (!is_dec) rc = load_row(*this, top_tensors<Ctx<T>>(), name.c_str(), false, name, data, shape, ndim);
    else if ((rc = load_row(dec[l], block_tensors<T>(), part, true, name, data, shape, ndim)) == -1)
      rc = load_row(dec[l], cross_tensors<T>(), part, true, name, data, shape, ndim);
    if (rc) return rc == -1 ? fail(-5, "unknown tensor " + name) : rc;
    loaded.insert(name);
    // what finalize() derives from the weights (wqx_f, the 8-bit encoder, decoder and vocabulary weights) is
    // stale now
    finalized = false;
    e8_quantised = false;
    d8_quantised = false;
    v8_quantised = false;
    return 0;
  }

  int finalize() override {
    const size_t expected = n_loadable<Ctx<T>>(La, Ld);
    if (loaded.size() != expected)
      return fail(-6, "loaded " + std::to_string(loaded.size()) + " of " + std::to_string(expected) + " tensors");
    // the fragment-ordered W_q copies (after the 0.125 query scale was folded in at load)
    for (auto& e : dec)
      if (e.wqx_f) launch_wq_frag(e.wqx, e.wqx_f, ns, st);
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    finalized = true;
    if (enc_fmt == WH_ENC_FP8_E4M3) TRY(quantise_enc8());
    // (w8_step: a batch begun in fp8 still reads the copies after the format was set back)
    if (dec_fmt == WH_DEC_FP8_E4M3 || w8_step) TRY(quantise_dec8());
    if (vocab_fmt == WH_VOCAB_FP8_E4M3 || v8_step) TRY(quantise_vocab8());
    return 0;
  }

  // ------------------------------------------------------------ vocabulary format
  int quantise_vocab8() {
    if (launch_quant_vocab_w8(E, v8_codes, v8_scales, V, ns, st))
      return fail(-20, "vocab_format: k_quant_vocab_w8 does not serve n_text_state " + std::to_string(ns));
    HIPCHK(hipStreamSynchronize(st));
    TRY(launch_status(__func__));
    v8_quantised = true;
    return 0;
  }
  int set_vocab_format(int fmt) override {
    if (fmt != WH_VOCAB_NATIVE && fmt != WH_VOCAB_FP8_E4M3)
      return fail(-12, "vocab_format: unknown format " + std::to_string(fmt));
    if (fmt == vocab_fmt) return 0;
    if (fmt == WH_VOCAB_FP8_E4M3) {
      if (sizeof(T) != 2) return fail(-12, "vocab_format: WH_VOCAB_FP8_E4M3 needs an fp16 context (this one is fp32)");
      if (!proj1_supported(1, ns) || !v8_kw(ns))
        return fail(-12, "vocab_format: WH_VOCAB_FP8_E4M3 serves n_text_state 1280, 1024, 768, 512, 384 and 128 (the "
                         "single-window step kernel's widths), not " + std::to_string(ns));
      if (!v8_codes) {
        const size_t cb = (size_t)v8_cols(V) * ns;  // (a multiple of 16 bytes: the scales behind it are aligned)
        void* p = nullptr;
        HIPCHK(hipMalloc(&p, cb + (size_t)v8_cols(V) * 4));
        v8_codes = (uint8_t*)p;
        v8_scales = (float*)(v8_codes + cb);
      }
      if (finalized && !v8_quantised) TRY(quantise_vocab8());
    }
    // (the captured step graph holds the kernels of v8_step, the format of the batch in flight:
    // begin_batch drops it where the next batch begins in the other format)
    vocab_fmt = fmt;
    return 0;
  }
  int read_vocab_w8(uint8_t* codes, float* scales) override {
    if (vocab_fmt != WH_VOCAB_FP8_E4M3) return fail(-12, "read_vocab_w8: the context's vocabulary format is WH_VOCAB_NATIVE");
    if (!finalized) return fail(-9, "read_vocab_w8: weights not finalized");
    std::vector<uint8_t> h((size_t)v8_cols(V) * ns);
    HIPCHK(hipMemcpy(h.data(), v8_codes, h.size(), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(scales, v8_scales, (size_t)V * 4, hipMemcpyDeviceToHost));
    const int sw = v8_sw(ns);
    for (int r = 0; r < V; ++r)
      for (int k = 0; k < ns; ++k) codes[(size_t)r * ns + k] = h[v8_offset(r, k, ns, sw)];
    return 0;
  }

  // ------------------------------------------------------------ decoder format
  const T* dec_weight(int l, int which) const {
    const auto& e = dec[l];
    const T* w[6] = {e.wqkv, e.wo, e.wqx, e.wox, e.w1, e.w2};
    return w[which];
  }
  int quantise_dec8() {
    for (int l = 0; l < Ld; ++l)
      for (int i = 0; i < 6; ++i)
        if (launch_quant_dec_w8(dec_weight(l, i), dec8[l].w[i], dec8[l].s[i], (int)DEC8_OUT[i] * ns, (int)DEC8_IN[i] * ns,
                                p1_nstep(ns), st))
          return fail(-20, "decoder_format: k_quant_dec_w8 does not serve n_text_state " + std::to_string(ns));
    HIPCHK(hipStreamSynchronize(st));
    TRY(launch_status(__func__));
    d8_quantised = true;
    return 0;
  }
  int set_dec_format(int fmt) override {
    if (fmt != WH_DEC_NATIVE && fmt != WH_DEC_FP8_E4M3)
      return fail(-12, "decoder_format: unknown format " + std::to_string(fmt));
    if (fmt == dec_fmt) return 0;
    if (fmt == WH_DEC_FP8_E4M3) {
      if (sizeof(T) != 2) return fail(-12, "decoder_format: WH_DEC_FP8_E4M3 needs an fp16 context (this one is fp32)");
      if (!proj1_supported(1, ns))
        return fail(-12, "decoder_format: WH_DEC_FP8_E4M3 serves n_text_state 1280, 1024, 768, 512, 384 and 128 (the "
                         "single-window step kernel's widths), not " + std::to_string(ns));
      if (!d8_base) {
        Arena ar;
        void* p = nullptr;
        const int rc = carve(&p, ar, [&](Arena& a) { layout_dec8(*this, a, ld); }, "decoder_format: 8-bit");
        d8_base = (char*)p;
        if (rc) return rc;
      }
      if (finalized && !d8_quantised) TRY(quantise_dec8());
    }
    // (the captured step graph holds the kernels of w8_step, the format of the batch in flight:
    // begin_batch drops it where the next batch begins in the other format)
    dec_fmt = fmt;
    return 0;
  }
  int read_dec_w8(int layer, int which, uint8_t* codes, float* scales) override {
    if (dec_fmt != WH_DEC_FP8_E4M3) return fail(-12, "read_decoder_w8: the context's decoder format is WH_DEC_NATIVE");
    if (!finalized) return fail(-9, "read_decoder_w8: weights not finalized");
    if (layer < 0 || layer >= Ld || which < 0 || which > 5) return fail(-12, "read_decoder_w8: bad layer or which");
    const int N = (int)DEC8_OUT[which] * ns, K = (int)DEC8_IN[which] * ns, nst = p1_nstep(ns);
    std::vector<uint8_t> h((size_t)N * K);
    HIPCHK(hipMemcpy(h.data(), dec8[layer].w[which], h.size(), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(scales, dec8[layer].s[which], (size_t)N * 4, hipMemcpyDeviceToHost));
    for (int r = 0; r < N; ++r)
      for (int k = 0; k < K; ++k) codes[(size_t)r * K + k] = h[(size_t)r * K + w8_offset(k, nst)];
    return 0;
  }
  // the 8-bit operands of layer l's projection `which` where this batch's single-window step
  // reads them; nulls: the fp16 weight
  struct W8 {
    const uint8_t* c = nullptr;
    const float* s = nullptr;
  };
  W8 w8(int l, int which) const { return w8_step ? W8{dec8[l].w[which], dec8[l].s[which]} : W8{}; }

  // ------------------------------------------------------------ encoder format
  int quantise_enc8() {
    const int n = ns;
    for (int l = 0; l < La; ++l) {
      const auto& e = enc[l];
      const auto& q = enc8[l];
      launch_quant_weights(e.wqkv, q.wqkv, q.sqkv, 3 * n, n, st);
      launch_quant_weights(e.wo, q.wo, q.so, n, n, st);
      launch_quant_weights(e.w1, q.w1, q.s1, 4 * n, n, st);
      launch_quant_weights(e.w2, q.w2, q.s2, n, 4 * n, st);
    }
    HIPCHK(hipStreamSynchronize(st));
    TRY(launch_status(__func__));
    e8_quantised = true;
    return 0;
  }
  // the 8-bit weights of every layer, then the codes + row scales of one GEMM input
  void layout_enc8(Arena& ar) {
    const size_t n = ns;
    enc8.resize(La);
    for (auto& q : enc8) {
      q.wqkv = ar.take<uint8_t>(3 * n * n); q.wo = ar.take<uint8_t>(n * n);
      q.w1 = ar.take<uint8_t>(4 * n * n); q.w2 = ar.take<uint8_t>(4 * n * n);
      q.sqkv = ar.take<float>(3 * n); q.so = ar.take<float>(n);
      q.s1 = ar.take<float>(4 * n); q.s2 = ar.take<float>(n);
    }
    e8x = ar.take<uint8_t>(ld.WE * 1500 * 4 * n);
    e8s = ar.take<float>(ld.WE * 1500);
  }
  int set_enc_format(int fmt) override {
    if (fmt != WH_ENC_NATIVE && fmt != WH_ENC_FP8_E4M3)
      return fail(-12, "encoder_format: unknown format " + std::to_string(fmt));
    if (fmt == WH_ENC_FP8_E4M3 && sizeof(T) != 2)
      return fail(-12, "encoder_format: WH_ENC_FP8_E4M3 needs an fp16 context (this one is fp32)");
    if (fmt == WH_ENC_FP8_E4M3 && !e8_base) {
      Arena ar;
      void* p = nullptr;
      const int rc = carve(&p, ar, [&](Arena& a) { layout_enc8(a); }, "encoder_format: 8-bit");
      e8_base = (char*)p;
      if (rc) return rc;
    }
    if (fmt == WH_ENC_FP8_E4M3 && finalized && !e8_quantised) TRY(quantise_enc8());
    enc_fmt = fmt;
    return 0;
  }
  // the tile kernel of each of the block's four GEMMs for an encode of n_win windows (native:
  // launch_gemm_tiles' rule for M > 128 rows)
  std::string encoder_kernels(int n_win) const override {
    const int n = ns, M = std::min(std::max(n_win, 1), std::min(Wcap, enc_chunk())) * 1500;
    const bool e8 = enc_fmt == WH_ENC_FP8_E4M3;
    auto name = [&](int N, int K) -> std::string {
      if (e8) return gemm8_tile(M, N, K) == 256 ? "k_gemm8<256x128>" : "k_gemm8<128x64>";
      const bool t256 = sizeof(T) == 2 && N % 256 == 0 && K % 128 == 0 && ((M + 255) / 256) * (N / 256) >= 256;
      return t256 ? "k_gemm_256" : "k_gemm_tile";
    };
    return std::string("encoder=") + (e8 ? "fp8" : "native") + ",qkv=" + name(3 * n, n) + ",out=" + name(n, n) +
           ",fc1=" + name(4 * n, n) + ",fc2=" + name(n, 4 * n);
  }
  int fp8_linear(int M, int N, int K, const float* x, const float* w, const float* bias, int gelu, int tile, float* y,
                 uint8_t* xc, float* xs, uint8_t* wc, float* ws) override {
    if (sizeof(T) != 2) return fail(-12, "fp8_linear: needs an fp16 context (this one is fp32)");
    if (M < 1 || N < 1 || K < 1 || !x || !w || !y || !xc || !xs || !wc || !ws) return fail(-12, "fp8_linear: bad arguments");
    if (K % G8_BK || K > 8192)
      return fail(-12, "fp8_linear: K=" + std::to_string(K) + " is not a multiple of the K-tile (128) up to 8192");
    if (tile != 0 && tile != 256 && tile != 128) return fail(-12, "fp8_linear: tile " + std::to_string(tile) + ": 0, 256 or 128");
    const int tl = tile ? tile : (N % 64 ? 256 : gemm8_tile(M, N, K)), cols = tl == 256 ? 128 : 64;
    if (N % cols)
      return fail(-12, "fp8_linear: N=" + std::to_string(N) + " is not a multiple of the tile's " + std::to_string(cols) + " columns");
    struct Dev {
      void* p = nullptr;
      ~Dev() { if (p) (void)hipFree(p); }
    } dev;
    const size_t mk = (size_t)M * K, nk = (size_t)N * K, mn = (size_t)M * N;
    half_t *dx, *dw, *dy;
    uint8_t *dxc, *dwc;
    float *dxs, *dws, *db;
    Arena ar;
    TRY(carve(&dev.p, ar, [&](Arena& a) {
      dx = a.take<half_t>(mk); dw = a.take<half_t>(nk);
      dxc = a.take<uint8_t>(mk); dwc = a.take<uint8_t>(nk);
      dxs = a.take<float>(M); dws = a.take<float>(N);
      db = a.take<float>(N); dy = a.take<half_t>(mn);
    }, "fp8_linear:"));
    std::vector<half_t> h(std::max(mk, std::max(nk, mn)));
    for (size_t i = 0; i < mk; ++i) h[i] = (half_t)x[i];
    HIPCHK(hipMemcpy(dx, h.data(), mk * 2, hipMemcpyHostToDevice));
    for (size_t i = 0; i < nk; ++i) h[i] = (half_t)w[i];
    HIPCHK(hipMemcpy(dw, h.data(), nk * 2, hipMemcpyHostToDevice));
    if (bias) HIPCHK(hipMemcpy(db, bias, (size_t)N * 4, hipMemcpyHostToDevice));
    launch_quant_rows(dx, dxc, dxs, M, K, st);
    launch_quant_weights(dw, dwc, dws, N, K, st);
    GemmArgs a;
    a.X = dxc; a.ldx = K; a.W = dwc; a.bias = bias ? db : nullptr; a.M = M; a.N = N; a.K = K;
    a.x_group_rows = M; a.out = dy; a.ldo = N;
    const int rc = launch_gemm8(a, dxs, dws, gelu ? EPI_STORE_GELU : EPI_STORE, tl, st);
    if (rc) return fail(-20, "fp8_linear: gemm8 launch failed code " + std::to_string(rc));
    HIPCHK(hipStreamSynchronize(st));
    TRY(launch_status(__func__));
    HIPCHK(hipMemcpy(h.data(), dy, mn * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < mn; ++i) y[i] = (float)h[i];
    HIPCHK(hipMemcpy(xc, dxc, mk, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(wc, dwc, nk, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(xs, dxs, (size_t)M * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ws, dws, (size_t)N * 4, hipMemcpyDeviceToHost));
    return 0;
  }

  // ------------------------------------------------------------ GEMM helper
  int gemm(const void* X, int ldx, const T* W, const float* bias, int M, int N, int K, int epi, GemmArgs a) {
    a.X = X; a.ldx = ldx; a.W = W; a.bias = bias; a.M = M; a.N = N; a.K = K;
    if (a.x_group_rows == (1 << 30)) a.x_group_rows = std::max(M, 1);
    const int rc = launch_gemm<T>(a, epi, st);
    if (rc) return fail(-20, "gemm launch failed code " + std::to_string(rc) + " M=" + std::to_string(M) +
                                 " N=" + std::to_string(N) + " K=" + std::to_string(K));
    return 0;
  }

  // ------------------------------------------------------------ encoder
  // single: the encode is ONE window (its decode batch runs the single-window path too):
  // the residual GEMMs (conv2, out, fc2) split K in two halves inside the launch — within
  // the fp16 bound of the multi-window encoder, not bit-equal to it, as k_proj1 in the step
  int encode_chunk(int s0, int we, bool single = false) {
    const int n = ns;
    GemmArgs g;
    const bool kz = single && we == 1 && sizeof(T) == 2 && !(tune_env("WHISPER_HIP_ENC_KZ") && tune_env("WHISPER_HIP_ENC_KZ")[0] == '0');
    auto kz_on = [&](GemmArgs& ga) {
      if (!kz) return;
      ga.p1_slab = ekz_slab;
      ga.p1_cnt = ekz_cnt;
      ga.p1_slabs = EKZ_TILES(n) * 64;
    };
    // mel windows -> time-major (T), conv1 as overlapping-row GEMM (lda = n_mels)
    const MelView mel = audio.mel();
    launch_mel_windows<T>(mel.p, mel.frames, n_mels, d_seeks + s0, d_segs + s0, melT, (int64_t)MROWS * n_mels, MROWS, we, st);
    g = GemmArgs();
    g.x_group_rows = 3000; g.x_group_stride = (int64_t)MROWS * n_mels;
    g.out = h1; g.ldo = n; g.out_group_stride = (int64_t)H1ROWS * n; g.out_row_off = 1;
    TRY(gemm(melT, n_mels, conv1_w, conv1_b, we * 3000, n, K1p, EPI_STORE_GELU, g));
    launch_zero_rows<T>(h1, (int64_t)H1ROWS * n, n, 0, H1ROWS - 1, we, st);
    // conv2 (stride 2): row t reads padded rows 2t..2t+2 -> lda = 2n; + GELU + positional embedding
    g = GemmArgs();
    g.x_group_rows = 1500; g.x_group_stride = (int64_t)H1ROWS * n;
    g.out_f32 = x_e; g.ldo = n; g.pos = pos_enc;
    kz_on(g);
    TRY(gemm(h1, 2 * n, conv2_w, conv2_b, we * 1500, n, 3 * n, EPI_GELU_POS, g));
    const int M = we * 1500;
    // WH_ENC_FP8_E4M3: the four GEMMs read codes + row scales (e8x, e8s: one input at a time,
    // the stream orders its writer behind the GEMM before it) and the layer's 8-bit weights
    const bool e8 = enc_fmt == WH_ENC_FP8_E4M3;
    auto gemm8 = [&](const uint8_t* Wc, const float* sw, const float* bias, int N, int K, int epi, GemmArgs a) -> int {
      a.X = e8x; a.ldx = K; a.W = Wc; a.bias = bias; a.M = M; a.N = N; a.K = K;
      if (a.x_group_rows == (1 << 30)) a.x_group_rows = M;
      const int rc = launch_gemm8(a, e8s, sw, epi, 0, st);
      if (rc) return fail(-20, "gemm8 launch failed code " + std::to_string(rc) + " M=" + std::to_string(M) +
                                   " N=" + std::to_string(N) + " K=" + std::to_string(K));
      return 0;
    };
    for (int l = 0; l < La; ++l) {
      auto& e = enc[l];
      if (e8) {
        const auto& q = enc8[l];
        launch_layernorm_quant(x_e, e8x, e8s, e.ln1_g, e.ln1_b, M, n, 1e-7f, st);
        g = GemmArgs(); g.out = qkv_e; g.ldo = 3 * n;
        g.x_group_rows = 1500; g.out_group_stride = (int64_t)1500 * 3 * n;
        g.hs_state = n; g.hs_heads = nh; g.hs_T = TKP; g.vc = vt_e;
        TRY(gemm8(q.wqkv, q.sqkv, e.bqkv, 3 * n, n, EPI_QKV_ENC, g));
        launch_attn_enc<T>(qkv_e, 3 * n, n, nh, 1500, we, (int64_t)1500 * 3 * n, vt_e, TKP, att_e, (int64_t)1500 * n, st);
        launch_quant_rows(att_e, e8x, e8s, M, n, st);
        g = GemmArgs(); g.out_f32 = x_e; g.ldo = n;
        TRY(gemm8(q.wo, q.so, e.bo, n, n, EPI_RESID, g));
        launch_layernorm_quant(x_e, e8x, e8s, e.ln2_g, e.ln2_b, M, n, 1e-7f, st);
        g = GemmArgs(); g.out = hm_e; g.ldo = 4 * n;
        TRY(gemm8(q.w1, q.s1, e.b1, 4 * n, n, EPI_STORE_GELU, g));
        launch_quant_rows(hm_e, e8x, e8s, M, 4 * n, st);
        g = GemmArgs(); g.out_f32 = x_e; g.ldo = n;
        TRY(gemm8(q.w2, q.s2, e.b2, n, 4 * n, EPI_RESID, g));
        continue;
      }
      launch_layernorm<T>(x_e, xn_e, e.ln1_g, e.ln1_b, M, n, 1e-7f, nullptr, st);
      // q, k -> qkv_e; v -> vt_e as per-(window, head) V^T with permuted keys
      g = GemmArgs(); g.out = qkv_e; g.ldo = 3 * n;
      g.x_group_rows = 1500; g.x_group_stride = (int64_t)1500 * n; g.out_group_stride = (int64_t)1500 * 3 * n;
      g.hs_state = n; g.hs_heads = nh; g.hs_T = TKP; g.vc = vt_e;
      TRY(gemm(xn_e, n, e.wqkv, e.bqkv, M, 3 * n, n, EPI_QKV_ENC, g));
      launch_attn_enc<T>(qkv_e, 3 * n, n, nh, 1500, we, (int64_t)1500 * 3 * n, vt_e, TKP, att_e, (int64_t)1500 * n, st);
      g = GemmArgs(); g.out_f32 = x_e; g.ldo = n;
      kz_on(g);
      TRY(gemm(att_e, n, e.wo, e.bo, M, n, n, EPI_RESID, g));
      launch_layernorm<T>(x_e, xn_e, e.ln2_g, e.ln2_b, M, n, 1e-7f, nullptr, st);
      g = GemmArgs(); g.out = hm_e; g.ldo = 4 * n;
      TRY(gemm(xn_e, n, e.w1, e.b1, M, 4 * n, n, EPI_STORE_GELU, g));
      g = GemmArgs(); g.out_f32 = x_e; g.ldo = n;
      kz_on(g);
      TRY(gemm(hm_e, 4 * n, e.w2, e.b2, M, n, 4 * n, EPI_RESID, g));
    }
    T* xa_s = xa + (size_t)s0 * 1500 * n;
    launch_layernorm<T>(x_e, xa_s, lnp_g, lnp_b, M, n, 1e-7f, nullptr, st);
    // cross-KV for every decoder layer in one GEMM, written head-split [l2][slot][h][t][64]
    g = GemmArgs();
    g.x_group_rows = 1500; g.x_group_stride = (int64_t)1500 * n;
    g.out = ckv; g.hs_state = n; g.hs_heads = nh; g.hs_T = TKP; g.hs_nslots = Wcap; g.hs_slot0 = s0;
    TRY(gemm(xa_s, n, ckv_w, ckv_b, M, 2 * Ld * n, n, EPI_HEADSPLIT, g));
    if (ckv8) launch_ckv_quant(ckv, ckv8, Ld, Wcap, s0, we, nh, st);
    return 0;
  }

  int encode(int n_win, const int64_t* seeks, const int* segs) override {
    if (!finalized) return fail(-9, "weights not finalized");
    if (n_win < 1 || n_win > Wcap) return fail(-9, "n_win out of range");
    const MelView mel = audio.mel();
    if (!mel.p || mel.n_mels != n_mels) return fail(-9, "no mel of the model's n_mels in the context");
    // seeks are absolute frames; the stored mel starts at mel.f0
    h_seeks.resize(n_win);
    for (int i = 0; i < n_win; ++i) {
      const int64_t s = seeks[i] - mel.f0;
      if (s < 0 || segs[i] < 1 || s + std::min(segs[i], 3000) > mel.frames) return fail(-9, "bad window");
      h_seeks[i] = s;
    }
    encoded = true;
    TRY(tm.mark(0, st));
    HIPCHK(hipMemcpyAsync(d_seeks, h_seeks.data(), n_win * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_segs, segs, n_win * 4, hipMemcpyHostToDevice, st));
    const int WE = std::min(Wcap, enc_chunk());
    for (int s0 = 0; s0 < n_win; s0 += WE) TRY(encode_chunk(s0, std::min(WE, n_win - s0), n_win == 1));
    TRY(tm.finish(st, stats[WH_STAT_ENCODE_MS]));
    stats[WH_STAT_ENCODE_WINDOWS] += n_win;
    TRY(launch_status(__func__));
    return 0;
  }

  int read_xa(int slot, float* out) override {
    if (slot < 0 || slot >= Wcap) return fail(-10, "slot");
    const size_t cnt = (size_t)1500 * ns;
    std::vector<T> h(cnt);
    HIPCHK(hipMemcpy(h.data(), xa + (size_t)slot * cnt, cnt * sizeof(T), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < cnt; ++i) out[i] = (float)h[i];
    return 0;
  }
  int read_ckv(int slot, int layer, float* k, float* v) override {
    if (slot < 0 || slot >= Wcap || layer < 0 || layer >= Ld) return fail(-10, "slot/layer");
    const size_t per = (size_t)nh * TKP * 64;
    std::vector<T> h(per);
    for (int kv = 0; kv < 2; ++kv) {
      const T* src = ckv + ((size_t)(2 * layer + kv) * Wcap + slot) * per;
      HIPCHK(hipMemcpy(h.data(), src, per * sizeof(T), hipMemcpyDeviceToHost));
      float* o = kv ? v : k;
      for (int hh = 0; hh < nh; ++hh)
        for (int t = 0; t < 1500; ++t) {
          // K: [H][TKP][64]; V: transposed, tile-major with the 32-key permutation (xv_index)
          for (int dd = 0; dd < 64; ++dd)
            o[((size_t)hh * 1500 + t) * 64 + dd] =
                kv ? (float)h[(size_t)hh * 64 * TKP + xv_index(dd, t)] : (float)h[((size_t)hh * TKP + t) * 64 + dd];
        }
    }
    return 0;
  }

  int set_ckv_format(int fmt) override {
    if (fmt != WH_CKV_NATIVE && fmt != WH_CKV_FP8_E4M3)
      return fail(-12, "cross_kv_format: unknown format " + std::to_string(fmt));
    if (fmt == (ckv8 ? WH_CKV_FP8_E4M3 : WH_CKV_NATIVE)) return 0;
    if (encoded) return fail(-12, "cross_kv_format: the format is fixed by the first wh_encode");
    if (fmt == WH_CKV_NATIVE) {
      HIPCHK(hipFree(ckv8));
      ckv8 = nullptr;
      return 0;
    }
    if (sizeof(T) != 2) return fail(-12, "cross_kv_format: WH_CKV_FP8_E4M3 needs an fp16 context (this one is fp32)");
    const size_t bytes = (size_t)Ld * Wcap * ckv8_slot_bytes(nh);
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, bytes));
    if (hipMemset(p, 0, bytes) != hipSuccess) {
      (void)hipFree(p);
      return fail(-100, "cross_kv_format: hipMemset failed");
    }
    ckv8 = (char*)p;
    return 0;
  }
  int read_ckv8(int slot, int layer, uint8_t* kc, float* ks, uint8_t* vc, float* vs) override {
    if (!ckv8) return fail(-12, "read_cross_kv8: the context's cross-KV format is WH_CKV_NATIVE");
    if (slot < 0 || slot >= Wcap || layer < 0 || layer >= Ld) return fail(-10, "slot/layer");
    std::vector<char> h(ckv8_slot_bytes(nh));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(h.data(), (const char*)kv8_layer(layer) + (size_t)slot * h.size(), h.size(), hipMemcpyDeviceToHost));
    for (int hh = 0; hh < nh; ++hh)
      for (int t = 0; t < 1500; ++t) {
        const char* rec = h.data() + ((size_t)hh * CKV8_TILES + t / 64) * CKV8_REC;
        const int kk = t & 63;
        const size_t o = (size_t)hh * 1500 + t;
        memcpy(&ks[o], rec + 8192 + 4 * kk, 4);
        memcpy(&vs[o], rec + 8448 + 4 * kk, 4);
        const int vpos = xv_perm(kk);  // the key's position in the fp16 V^T rows
        for (int dd = 0; dd < 64; ++dd) {
          // a row's byte 16 g + 8 s + e holds element 32 s + 8 g + e (wh_kernels.h CKV8_REC)
          auto at = [](int c) { return 16 * ((c >> 3) & 3) + 8 * (c >> 5) + (c & 7); };
          kc[o * 64 + dd] = (uint8_t)rec[kk * 64 + at(dd)];
          vc[o * 64 + dd] = (uint8_t)rec[4096 + dd * 64 + at(vpos)];
        }
      }
    return 0;
  }

  // ------------------------------------------------------------ decoder layers
  // R rows of x_d (f32 residual); rw/rs/rp: row window / beam slot / position
  // ancG: beams per window in the anc table layout [w][ancG][ctx]; KV slots use Gcap
  // residual projection x += X W^T + b, then xn = LayerNorm(x) with the NEXT norm's
  // parameters.  Up to 128 rows: split-K weight streaming into fp32 partial slabs,
  // summed in fixed order by k_resid_ln (deterministic, no atomics).  More rows:
  // tile GEMM with an in-place residual epilogue.
  // how many [R][N] fp32 slabs fit in the partial buffer
  int part_slabs(int R, int N) const { return (int)std::min<int64_t>(16, (int64_t)RSPLIT * RD * ns / ((int64_t)R * N)); }

  // X[R][K] W^T into the split-K partial slabs part[z][R][N]: k_proj where a tile
  // configuration fits (decode rows <= 112), the k_gemv path otherwise; *ks = z
  // fp16 contexts store the slabs as fp16 (slab_h = 1 after such a partial(); the QKV
  // projection's too unless WHISPER_HIP_SLAB16_QKV=0, slab16_qkv below): half the bytes
  // written by every k_proj and read by k_resid_ln / k_reduce_store / k_xattn_seg.  Round 4
  // measured 0.3 % and kept fp32; after round 5's issue-side fixes the 20-window step graph
  // is 3.378 -> 3.276 ms (early) and 3.661 -> 3.559 ms (150 tokens) with it
  // (profiles/r05/ab_slab16.txt), the fp16 teacher-forced / invariance tests unchanged.
  // Partial sums rounded to fp16 (the reference's CoreML path is fp16 end to end; the
  // residual stream here stays fp32).  Tuning build: WHISPER_HIP_SLAB16=0 keeps fp32 slabs.
  int slab_h = 0;
  static bool slab16_enabled() {
    static const bool on = [] {
      const char* e = tune_env("WHISPER_HIP_SLAB16");
      return !(e && e[0] == '0');
    }();
    return on;
  }
  // the QKV projection's slabs (read by k_self_attn_qkv<T, half_t>) fp16 too:
  // 20-window step graph 3.261 / 3.258 -> 3.255 / 3.246 ms, 3.557 -> 3.546 at 150 tokens
  // (profiles/r05/ab_slab16_qkv.txt).  Tuning build: WHISPER_HIP_SLAB16_QKV=0 keeps them fp32
  static bool slab16_qkv() {
    static const bool on = [] {
      const char* e = tune_env("WHISPER_HIP_SLAB16_QKV");
      return !(e && e[0] == '0');
    }();
    return on;
  }
  int partial(const void* X, int ldx, const T* W, int R, int N, int K, int* ks, bool half_ok = true) {
    GemmArgs g;
    g.X = X; g.ldx = ldx; g.W = W; g.M = R; g.N = N; g.K = K; g.x_group_rows = R;
    g.out_f32 = part; g.ldo = N;
    g.slab_half = half_ok && sizeof(T) == 2 && slab16_enabled();
    slab_h = g.slab_half;
    const int maxz = part_slabs(R, N);
    // time_stage(7): each k_proj of an eager step timed by its own dispatch events
    const bool tev = proj_ev_n < (int)proj_ev.size() / 2;
    const int rc = tev ? launch_proj_partial<T>(g, maxz, st, ks, proj_ev[2 * proj_ev_n], proj_ev[2 * proj_ev_n + 1])
                       : launch_proj_partial<T>(g, maxz, st, ks);
    if (tev && rc == 0) ++proj_ev_n;
    if (rc == 0) return 0;
    if (rc != -1) return fail(-20, "k_proj launch failed code " + std::to_string(rc));
    slab_h = 0;
    *ks = gemv_ksplit(R, N, K, maxz);
    g = GemmArgs();
    g.out_f32 = part; g.ldo = N; g.ksplit = *ks;
    return gemm(X, ldx, W, nullptr, R, N, K, EPI_PARTIAL, g);
  }

  int resid(const T* X, int K, const T* W, const float* b, int R, const float* lg, const float* lb) {
    const int n = ns;
    GemmArgs g;
    if (R > 128) {
      g.out_f32 = x_d; g.ldo = n;
      TRY(gemm(X, K, W, b, R, n, K, EPI_RESID, g));
      launch_resid_ln<T>(x_d, nullptr, 0, 0, nullptr, xn_d, lg, lb, R, n, 1e-5f, st);
    } else {
      int ks = 0;
      TRY(partial(X, K, W, R, n, K, &ks));
      launch_resid_ln<T>(x_d, part, ks, (int64_t)R * n, b, xn_d, lg, lb, R, n, 1e-5f, st, slab_h);
    }
    return 0;
  }
  // out = act(xn W^T + b) for R rows (cross-attention query, MLP fc1): split-K
  // partial slabs + fixed-order reduce in step mode, the direct GEMM otherwise
  int proj(const T* W, const float* b, int R, int N, T* out, int gelu, bool skinny) {
    GemmArgs g;
    if (skinny) {
      int ks = 0;
      TRY(partial(xn_d, ns, W, R, N, ns, &ks));
      launch_reduce_store<T>(part, ks, (int64_t)R * N, b, out, N, R, N, gelu, st, slab_h);
    } else {
      g.out = out; g.ldo = N;
      TRY(gemm(xn_d, ns, W, b, R, N, ns, gelu ? EPI_STORE_GELU : EPI_STORE, g));
    }
    return 0;
  }

  // R rows of x_d (embeddings in, residual stream out); on exit xn_d holds the final
  // decoder LayerNorm of every row (decoder.py:316) — except on the k_proj1 path
  // (dec_layers_p1), which leaves final_x set instead: vocab() computes that LayerNorm
  // in its prologue.
  // anc: the ancestry table the self-attention reads ([w][ancG][CTX]); the decode's S.anc
  // unless a first pass (alignment / prefill logits) gives its own (fp_anc: all zeros)
  int sa_probe_ks = 1;  // the QKV projection's split count (time_stage 8 / 9)
  int sa_probe_half = 0;  // and whether its slabs were fp16
  int dec_layers(int R, const int* rw, const int* rs, const int* rp, int ancG, int nwin, const int* wr0, const int* wnr,
                 const int* wsl, float* aqk, const int* qkmap, int qkrows, bool step = false,
                 const int* anc = nullptr) {
    const int* A = anc ? anc : S.anc;
    const int n = ns;
    // step mode (one row per beam, rows independent): the skinny projections run
    // split-K into fp32 partial slabs; QKV's reduction is fused into self-attention
    const bool skinny = step && R <= 128;
    GemmArgs g;
    final_x = nullptr;
    if (step && !qkmap && p1_active(R, nwin))
      return dec_layers_p1(R, rw, rs, rp, ancG, nwin, wr0, wnr, wsl, A);
    launch_layernorm<T>(x_d, xn_d, dec[0].ln1_g, dec[0].ln1_b, R, n, 1e-5f, nullptr, st);
    for (int l = 0; l < Ld; ++l) {
      auto& e = dec[l];
      if (skinny) {
        int ks = 0;
        TRY(partial(xn_d, n, e.wqkv, R, 3 * n, n, &ks, slab16_qkv()));
        sa_probe_ks = ks;
        sa_probe_half = slab_h;
        if (launch_self_attn_qkv<T>(part, ks, (int64_t)R * 3 * n, e.bqkv, n, kc[l], vc[l], rw, rs, rp, A, ancG,
                                    Gcap, nh, CTX, att_d, n, R, st, slab_h))
          return fail(-20, "self-attention rows are not a whole number of beam groups");
      } else {
        g = GemmArgs();
        g.out = q_d; g.ldo = n; g.hs_state = n; g.hs_heads = nh;
        g.row_win = rw; g.row_slot = rs; g.row_pos = rp; g.kc = kc[l]; g.vc = vc[l]; g.kv_beams = Gcap; g.kv_ctx = CTX;
        TRY(gemm(xn_d, n, e.wqkv, e.bqkv, R, 3 * n, n, EPI_QKV_DEC, g));
        launch_self_attn<T>(q_d, n, kc[l], vc[l], rw, rs, rp, A, ancG, Gcap, nh, CTX, att_d, n, R, st);
      }
      TRY(resid(att_d, n, e.wo, e.bo, R, e.lnx_g, e.lnx_b));
      // cross-attention query: in step mode its split-K slabs are reduced inside
      // k_cross_attn (rows per window <= Gcap <= 8), otherwise projected directly
      XQPart xq;
      if (skinny) xq = step_xq(ancG);
      if (skinny && xq_proj_active(ancG)) {
        // round 6: no cross-q launch; k_xattn_seg projects the LayerNorm'd rows itself
        xq.qx = xn_d; xq.qwf = e.wqx_f; xq.bias = e.bqx;
      } else if (skinny && xq_fused) {
        int ks = 0;
        TRY(partial(xn_d, n, e.wqx, R, n, n, &ks));
        if (cross_attn_q_slabs(ks)) {
          xq.part = part; xq.part_half = slab_h; xq.stride = (int64_t)R * n; xq.z = ks; xq.bias = e.bqx;
        } else {
          launch_reduce_store<T>(part, ks, (int64_t)R * n, e.bqx, q_d, n, R, n, 0, st, slab_h);
        }
      } else {
        TRY(proj(e.wqx, e.bqx, R, n, q_d, 0, skinny));
      }
      const T* ck = ckv + (size_t)(2 * l) * Wcap * TKP * n;
      const T* cv = ckv + (size_t)(2 * l + 1) * Wcap * TKP * n;
      launch_cross_attn<T>(q_d, n, ck, cv, 1500, nh, NSPLIT, nwin, wr0, wnr, wsl, (int64_t)TKP * n, po, pm, pl, att_d,
                           n, R, aqk, qkmap ? qkmap + l * nh : nullptr, qkrows, st, xq, skinny ? kv8_layer(l) : nullptr);
      TRY(resid(att_d, n, e.wox, e.box, R, e.ln2_g, e.ln2_b));
      TRY(proj(e.w1, e.b1, R, 4 * n, hm_d, 1, skinny));
      const bool last = l + 1 == Ld;
      TRY(resid(hm_d, 4 * n, e.w2, e.b2, R, last ? ln_g : dec[l + 1].ln1_g, last ? ln_b : dec[l + 1].ln1_b));
    }
    return 0;
  }

  // Decoder step at <= P1_RMAX rows (one window's beams: the per-token latency path):
  // every projection is one k_proj1 launch over the whole K with its epilogue fused
  // (QKV scatter, residual add, GELU) and the LayerNorm before it recomputed in its
  // prologue, so a layer is 8 launches: qkv, self-attn, out, cross-q, cross-attn,
  // cross-out, fc1, fc2 (12 on the split-K path: + 3 resid+LN, + reduce+GELU).
  // WHISPER_HIP_P1=0 keeps the split-K path (A/B).
  static bool p1_enabled() {
    static const bool on = [] {
      const char* e = tune_env("WHISPER_HIP_P1");
      return !(e && e[0] == '0');
    }();
    return on;
  }

  // q: the weight's 8-bit copy (w8()), which then stands in for g.W
  int p1(GemmArgs& g, int epi, bool ln, W8 q) {
    g.p1_slab = p1_slab;
    g.p1_cnt = p1_cnt;
    g.p1_slabs = P1_SLABS;
    // time_stage(7): each projection of an eager step timed by its own dispatch events
    const bool tev = proj_ev_n < (int)proj_ev.size() / 2;
    hipEvent_t e0 = tev ? proj_ev[2 * proj_ev_n] : nullptr, e1 = tev ? proj_ev[2 * proj_ev_n + 1] : nullptr;
    if (q.c) g.W = q.c;
    const int rc = q.c ? launch_proj1_w8(g, q.s, epi, ln, st, e0, e1) : launch_proj1<T>(g, epi, ln, st, e0, e1);
    if (tev && rc == 0) ++proj_ev_n;
    return rc == 0 ? 0 : fail(-20, "k_proj1 launch failed code " + std::to_string(rc));
  }

  // the six projections of layer l as the step issues them (p1 path: k_proj1 with the
  // step's epilogues; split path: k_proj into partial slabs) — time_stage(2)
  int layer_projections(int l, int R) {
    const int n = ns;
    auto& e = dec[l];
    if (p1_active(R, cur_nwin)) {
      GemmArgs g;
      g.W = e.wqkv; g.bias = e.bqkv; g.M = R; g.N = 3 * n; g.K = n;
      g.xf32 = x_d; g.ln_g = e.ln1_g; g.ln_b = e.ln1_b; g.ln_eps = 1e-5f;
      g.out = q_d; g.ldo = n; g.hs_state = n; g.hs_heads = nh;
      g.row_win = st_row_win; g.row_slot = st_row_slot; g.row_pos = row_pos; g.kc = kc[l]; g.vc = vc[l];
      g.kv_beams = Gcap; g.kv_ctx = CTX;
      TRY(p1(g, EPI_QKV_DEC, true, w8(l, 0)));
      struct Q { const T* X; int K; const T* W; const float* b; int N; int epi; const float* lg; const float* lb; T* out; };
      const Q qs[5] = {{att_d, n, e.wo, e.bo, n, EPI_RESID, nullptr, nullptr, nullptr},
                       {nullptr, n, e.wqx, e.bqx, n, EPI_STORE, e.lnx_g, e.lnx_b, q_d},
                       {att_d, n, e.wox, e.box, n, EPI_RESID, nullptr, nullptr, nullptr},
                       {nullptr, n, e.w1, e.b1, 4 * n, EPI_STORE_GELU, e.ln2_g, e.ln2_b, hm_d},
                       {hm_d, 4 * n, e.w2, e.b2, n, EPI_RESID, nullptr, nullptr, nullptr}};
      for (const Q& q : qs) {
        g = GemmArgs();
        g.W = q.W; g.bias = q.b; g.M = R; g.N = q.N; g.K = q.K;
        if (q.lg) {
          g.xf32 = x_d; g.ln_g = q.lg; g.ln_b = q.lb; g.ln_eps = 1e-5f; g.out = q.out; g.ldo = q.N;
        } else {
          g.X = q.X; g.ldx = q.K; g.out_f32 = x_d; g.ldo = n;
        }
        TRY(p1(g, q.epi, q.lg != nullptr, w8(l, 1 + (int)(&q - qs))));
      }
      return 0;
    }
    struct P { const T* X; int K; const T* W; int N; } ps[6] = {
        {xn_d, n, e.wqkv, 3 * n}, {att_d, n, e.wo, n}, {xn_d, n, e.wqx, n},
        {att_d, n, e.wox, n},     {xn_d, n, e.w1, 4 * n}, {hm_d, 4 * n, e.w2, n}};
    for (auto& p : ps) {
      if (p.W == e.wqx && xq_proj_active(cur_G)) continue;  // the step projects the cross-q in k_xattn_seg
      int ks = 0;
      TRY(partial(p.X, p.K, p.W, R, p.N, p.K, &ks));
    }
    return 0;
  }

  // the k_proj1 layers serve exactly one window (its beams, <= P1_RMAX rows): the cut is a
  // window count, not a row count, so a window's step arithmetic is the same in every
  // batch of >= 2 windows whatever the beam count (greedy included; batch invariance,
  // DESIGN.md §2)
  bool p1_active(int R, int n_win) const { return n_win == 1 && p1_enabled() && proj1_supported(R, ns); }
  std::string step_kernels(int n_win, int group) const override {
    const bool p1 = p1_active(n_win * group, n_win), h = sizeof(T) == 2;
    const bool qp = !p1 && xq_proj_active(group);
    // the 8-bit copy serves the steps k_xattn_seg serves: up to 128 rows (dec_layers: skinny);
    // a larger step runs the first-pass kernel over the fp16 cross-KV, in either format
    const bool kv8 = ckv8 && n_win * group <= 128;
    // vocab(): after the k_proj1 layers the final LayerNorm runs in the kernel's prologue, and
    // a batch begun now reads the 8-bit copy where the format is set
    const bool v8 = p1 && vocab_fmt == WH_VOCAB_FP8_E4M3;
    const VocabKernel vk = step_vocab_kernel((int)sizeof(T), n_win * group, V, ns, p1, v8);
    return std::string("proj=") + (p1 ? (dec_fmt == WH_DEC_FP8_E4M3 ? "k_proj1<w8>" : "k_proj1") : "k_proj") + ",xattn=k_xattn_seg" +
           (kv8 ? (qp ? "<kv8,qproj>" : "<kv8>") : qp ? "<qproj>" : "") + ",self_attn=" +
           (p1 ? (h ? "k_self_attn<kco>" : "k_self_attn") : h ? "k_self_attn_qkv<pipe+kco>" : "k_self_attn_qkv") +
           (v8 ? ",tail=vocab<w8>+k_logit_part" : ",tail=vocab+k_logit_part") + ",vocab=" + vocab_kernel_name(vk);
  }

  int dec_layers_p1(int R, const int* rw, const int* rs, const int* rp, int ancG, int nwin, const int* wr0,
                    const int* wnr, const int* wsl, const int* A) {
    const int n = ns;
    // deferred residual: fc2 stores its two K-half slabs only; the next layer's QKV
    // LayerNorm prologue adds them (+ bias) to the current rows and one of its workgroups
    // publishes the sum into the other buffer, which becomes current (fc2 7.9 -> 5.9 us,
    // the QKV prologue +0.6; profiles/r03/step_w1_p1def_summary.txt)
    float* xc = x_d;
    float* xo = x2_d;
    const float* pend = nullptr;  // bias of the residual pending in p1_slab
    auto ln_in = [&](GemmArgs& g, const float* lg, const float* lb) {
      g.xf32 = xc; g.ln_g = lg; g.ln_b = lb; g.ln_eps = 1e-5f;
      if (pend) { g.res_slab = p1_slab; g.res_bias = pend; g.x_out = xo; }
    };
    auto ln_done = [&]() {
      if (pend) { std::swap(xc, xo); pend = nullptr; }
    };
    auto resid = [&](const T* X, int K, const T* W, W8 q, const float* b, bool defer) -> int {
      GemmArgs g;
      g.X = X; g.ldx = K; g.W = W; g.bias = b; g.M = R; g.N = n; g.K = K; g.out_f32 = xc; g.ldo = n;
      g.p1_defer = defer;
      TRY(p1(g, EPI_RESID, false, q));
      if (defer) pend = b;
      return 0;
    };
    for (int l = 0; l < Ld; ++l) {
      auto& e = dec[l];
      // self-attention block: q, k, v of LN1(x) (k / v straight into the cache)
      GemmArgs g;
      g.W = e.wqkv; g.bias = e.bqkv; g.M = R; g.N = 3 * n; g.K = n;
      ln_in(g, e.ln1_g, e.ln1_b);
      g.out = q_d; g.ldo = n; g.hs_state = n; g.hs_heads = nh;
      g.row_win = rw; g.row_slot = rs; g.row_pos = rp; g.kc = kc[l]; g.vc = vc[l]; g.kv_beams = Gcap; g.kv_ctx = CTX;
      TRY(p1(g, EPI_QKV_DEC, true, w8(l, 0)));
      ln_done();
      launch_self_attn<T>(q_d, n, kc[l], vc[l], rw, rs, rp, A, ancG, Gcap, nh, CTX, att_d, n, R, st);
      TRY(resid(att_d, n, e.wo, w8(l, 1), e.bo, false));  // deferring it measured +1.0 us on cross-q, -0.2 here
      // cross-attention block
      XQPart xq = step_xq(ancG);
      g = GemmArgs();
      g.W = e.wqx; g.bias = e.bqx; g.M = R; g.N = n; g.K = n;
      ln_in(g, e.lnx_g, e.lnx_b);
      g.out = q_d; g.ldo = n;
      TRY(p1(g, EPI_STORE, true, w8(l, 2)));
      ln_done();
      const T* ck = ckv + (size_t)(2 * l) * Wcap * TKP * n;
      const T* cv = ckv + (size_t)(2 * l + 1) * Wcap * TKP * n;
      launch_cross_attn<T>(q_d, n, ck, cv, 1500, nh, NSPLIT, nwin, wr0, wnr, wsl, (int64_t)TKP * n, po, pm, pl, att_d,
                           n, R, nullptr, nullptr, 0, st, xq, kv8_layer(l));
      // (not deferred: fc1's 16-wave LayerNorm prologue has no registers for two more row copies)
      TRY(resid(att_d, n, e.wox, w8(l, 3), e.box, false));
      // MLP; the last layer's fc2 reduces in-launch (the final LayerNorm reads x)
      g = GemmArgs();
      g.W = e.w1; g.bias = e.b1; g.M = R; g.N = 4 * n; g.K = n;
      ln_in(g, e.ln2_g, e.ln2_b);
      g.out = hm_d; g.ldo = 4 * n;
      TRY(p1(g, EPI_STORE_GELU, true, w8(l, 4)));
      ln_done();
      TRY(resid(hm_d, 4 * n, e.w2, w8(l, 5), e.b2, l + 1 < Ld));
    }
    // the final LayerNorm runs in the vocabulary kernel's prologue (vocab(), final_x)
    final_x = xc;
    return 0;
  }

  // logits = LN(x) E^T for R rows of xn_d (optionally gathered by rows_sel)
  // (decoder.py:238-240, 316-320)
  // (after dec_layers_p1, final_x names the fp32 residual rows whose final LayerNorm
  // k_vocab_small computes itself: no separate LayerNorm launch per token)
  const float* final_x = nullptr;
  int vocab(const int* rows_sel, int R, float* out) {
    GemmArgs g;
    g.out_f32 = out; g.ldo = V; g.x_rows = rows_sel;
    // after dec_layers_p1, xn_d does not hold the final LayerNorm: only the prologue path
    // (every row, no gather) is valid there
    if (final_x && rows_sel) return fail(-20, "vocab: a row gather after the k_proj1 layers (xn_d not written)");
    if (final_x) {
      g.xf32 = final_x; g.ln_g = ln_g; g.ln_b = ln_b; g.ln_eps = 1e-5f;
    }
    // both launchers take their kernel from step_vocab_kernel (wh_vocab_pick.h), as step_kernels does
    if (final_x && v8_step) {  // this batch's single-window step reads the 8-bit copy of E
      g.W = v8_codes; g.M = R; g.N = V; g.K = ns;
      const int rc = launch_vocab1_w8(g, v8_scales, st);
      return rc == 0 ? 0 : fail(-20, "k_vocab1_w8 launch failed code " + std::to_string(rc));
    }
    return gemm(xn_d, ns, E, nullptr, R, V, ns, EPI_F32_COLS, g);
  }

  // ------------------------------------------------------------ decoding
  // The rows of a first pass through the decoder layers.  rows_dirty comes before the first
  // upload into row_pos / x_d: a failing copy must still make the next decode_steps re-embed
  // its rows.  The plan lives in the caller's frame until the caller has synchronised.
  // group / anc: the beams per window of the ancestry table the self-attention reads
  int run_rows(const RowPlan& p, int group, float* d_qk, const int* qkmap, int qk_rows, const int* anc) {
    rows_dirty = true;
    HIPCHK(hipMemcpyAsync(row_tok, p.row_tok.data(), p.R * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(row_pos, p.row_pos.data(), p.R * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(row_win, p.row_win.data(), p.R * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(row_slot, p.row_slot.data(), p.R * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(win_row0, p.win_row0.data(), p.nw() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(win_nrows, p.win_nrows.data(), p.nw() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(win_slot, p.win_slot.data(), p.nw() * 4, hipMemcpyHostToDevice, st));
    launch_embed<T>(E, Pdec, ns, row_tok, row_pos, nullptr, nullptr, 1, HCTX, CTX - 1, x_d, p.R, st);
    return dec_layers(p.R, row_win, row_slot, row_pos, group, p.nw(), win_row0, win_nrows, win_slot, d_qk, qkmap, qk_rows,
                      false, anc);
  }

  // the prompt pass of decode windows w0..w0+nw-1, all in beam slot 0; the logits of each
  // window's sot_index and last rows go to logits2.  (rows_dirty, which run_rows sets, changes
  // nothing here: decode_begin clears it right after, a per-step batch never reads it.)
  int prefill(int w0, int nw, const int* init, const int* n_init, int max_init, const int* sot_index) {
    RowPlan rows;
    std::vector<int> sel;
    for (int w = w0; w < w0 + nw; ++w) {
      rows.add(w, win_slots[w], init + (size_t)w * max_init, n_init[w]);
      sel.push_back(rows.win_row0.back() + sot_index[w]);
      sel.push_back(rows.win_row0.back() + n_init[w] - 1);
    }
    HIPCHK(hipMemcpyAsync(rows_in, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, st));
    TRY(run_rows(rows, S.G, nullptr, nullptr, 0, nullptr));
    TRY(vocab(rows_in, 2 * nw, logits2 + (size_t)2 * w0 * V));
    // the host vectors must outlive the async copies
    HIPCHK(hipStreamSynchronize(st));
    return 0;
  }

  // prefill of the initial tokens of n_win windows (G rows each, sharing beam slot 0 of
  // the self-KV), the decode state for step len = n_init[w], and the static step-row
  // metadata.  Leaves the sot_index / last-row logits of window w in logits2 rows
  // 2w / 2w+1 (and, when no_speech >= 0, its no-speech probability in nsp).
  // Window w reads the audio features / cross-KV of slot slots[w] (identity when null):
  // a temperature fallback decodes the windows that still need work straight from the
  // slots that hold them, without re-running the encoder.
  int begin_batch(int n_win, int G, const int* init, const int* n_init, int max_init, const int* sot_index,
                  int no_speech, const int* slots = nullptr) {
    TRY(begin_check(n_win, G, init, n_init, max_init, sot_index, slots));
    // host-side initial state
    std::vector<int> hist((size_t)n_win * Gcap * HCTX, 0), anc((size_t)n_win * Gcap * CTX, 0);
    const std::vector<int> nin(n_init, n_init + n_win);
    S.G = G;
    // history / ancestry laid out with the runtime group G ([w][G][..])
    for (int w = 0; w < n_win; ++w)
      for (int b = 0; b < G; ++b) {
        for (int p = 0; p < nin[w]; ++p) hist[((size_t)w * G + b) * HCTX + p] = init[(size_t)w * max_init + p];
        for (int p = 0; p < CTX; ++p) anc[((size_t)w * G + b) * CTX + p] = p < nin[w] ? 0 : b;
      }
    // prefill (anc must be in place first: prefill rows read slot 0 through it)
    HIPCHK(hipMemcpyAsync(S.anc, anc.data(), (size_t)n_win * G * CTX * 4, hipMemcpyHostToDevice, st));
    // prefill runs with kv_beams = Gcap layout; rows use slot 0
    for (int w0 = 0; w0 < n_win;) {
      int rows = 0, nw = 0;
      while (w0 + nw < n_win && (nw == 0 || rows + nin[w0 + nw] <= PRE)) rows += nin[w0 + nw++];
      if (rows > PRE) return fail(-11, "prefill rows exceed buffer");
      TRY(prefill(w0, nw, init, n_init, max_init, sot_index));
      w0 += nw;
    }
    // no_speech prob from the sot row of each window (decoding.py:716-720)
    if (no_speech >= 0) launch_no_speech(logits2, 2 * V, n_win, V, no_speech, nsp, st);
    // last-row logits replicated to the G rows of each window
    std::vector<int> src(n_win);
    for (int w = 0; w < n_win; ++w) src[w] = 2 * w + 1;
    HIPCHK(hipMemcpyAsync(src_rows, src.data(), n_win * 4, hipMemcpyHostToDevice, st));
    launch_broadcast_rows(logits2, V, src_rows, logits, V, G, n_win, V, st);
    // decode state
    HIPCHK(hipMemcpyAsync(S.hist, hist.data(), (size_t)n_win * G * HCTX * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(S.len, nin.data(), n_win * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(S.sample_begin, nin.data(), n_win * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(S.step, 0, n_win * 4, st));
    HIPCHK(hipMemsetAsync(S.done, 0, n_win * 4, st));
    HIPCHK(hipMemsetAsync(S.fin_n, 0, n_win * 4, st));
    HIPCHK(hipMemsetAsync(S.sum_lp, 0, n_win * G * 4, st));
    HIPCHK(hipMemcpyAsync(S.seed, &h_seed, 8, hipMemcpyHostToDevice, st));
    // static step-row metadata: row r = w*G + b
    std::vector<int> srw(n_win * G), srs(n_win * G), swr0(n_win), swnr(n_win, G), swsl(n_win);
    for (int w = 0; w < n_win; ++w) {
      swr0[w] = w * G;
      swsl[w] = win_slots[w];
      for (int b = 0; b < G; ++b) { srw[w * G + b] = w; srs[w * G + b] = b; }
    }
    HIPCHK(hipMemcpyAsync(st_row_win, srw.data(), srw.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(st_row_slot, srs.data(), srs.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(st_win_row0, swr0.data(), n_win * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(st_win_nrows, swnr.data(), n_win * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(st_win_slot, swsl.data(), n_win * 4, hipMemcpyHostToDevice, st));
    // the self-KV cache uses [w][Gcap][..] slots; the anc table uses [w][G][..]
    cur_nwin = n_win;
    cur_G = G;
    // a format set during the last batch serves from this one on; the captured step graph
    // holds the last batch's kernels and its key (wh_loop.hip ensure_graph) does not know
    // the format, so it goes where the format flips
    if (w8_step != (dec_fmt == WH_DEC_FP8_E4M3) || v8_step != (vocab_fmt == WH_VOCAB_FP8_E4M3)) {
      HIPCHK(hipStreamSynchronize(st));
      if (gexec) { HIPCHK(hipGraphExecDestroy(gexec)); gexec = nullptr; }
      if (graph) { HIPCHK(hipGraphDestroy(graph)); graph = nullptr; }
      w8_step = dec_fmt == WH_DEC_FP8_E4M3;
      v8_step = vocab_fmt == WH_VOCAB_FP8_E4M3;
    }
    h_len = nin;
    // the host vectors above must outlive the async copies
    HIPCHK(hipStreamSynchronize(st));
    return 0;
  }

  int decode_begin(int n_win, const wh_decode_opts* o, const int* init, const int* n_init, int max_init,
                   const int* sot_index, const int* slots) override {
    if (!finalized) return fail(-9, "weights not finalized");
    if (n_win < 1 || n_win > Wcap) return fail(-11, "n_win out of range");
    TRY(set_opts(o, n_win));
    TRY(tm.mark(0, st));
    TRY(begin_batch(n_win, o->group, init, n_init, max_init, sot_index, o->no_speech, slots));
    S.maxc = std::max(maxc, 1);
    maxc_stride = S.maxc;
    // first update on the prefill logits (decoding.py:713-733, i == 0); the merge also
    // embeds each row's new token: the first step's input rows
    launch_select_merge(logits, V, S, O, n_win, st, merge_embed());
    rows_dirty = false;
    return tm.finish(st, stats[WH_STAT_PREFILL_MS], __func__);
  }

  // re-embeds every step row from the decode state (S.hist, S.len) after other work went
  // through x_d / row_pos (wh_loop.h rows_dirty)
  void restore_rows() override {
    if (!rows_dirty || cur_nwin < 1 || step_api) return;
    launch_embed<T>(E, Pdec, ns, nullptr, row_pos, S.hist, S.len, cur_G, HCTX, CTX - 1, x_d, cur_nwin * cur_G, st);
    rows_dirty = false;
  }
  // k_merge writes the next step's input rows (x_d, row_pos): no k_embed launch per token
  MergeEmbed merge_embed() const {
    MergeEmbed em;
    em.E = E; em.P = Pdec; em.x = x_d; em.row_pos = row_pos; em.n = ns; em.pmax = CTX - 1; em.half = sizeof(T) == 2;
    return em;
  }
  // one decoder step for the current batch (graph body); its input rows were embedded by
  // the previous update's k_merge (decode_begin's first update for the first step)
  int step_body() override {
    const int R = cur_nwin * cur_G;
    TRY(dec_layers(R, st_row_win, st_row_slot, row_pos, cur_G, cur_nwin, st_win_row0, st_win_nrows, st_win_slot,
                   nullptr, nullptr, 0, true));
    TRY(vocab(nullptr, R, logits));
    launch_select_merge(logits, V, S, O, cur_nwin, st, merge_embed());
    return 0;
  }

  // ------------------------------------------------------------ per-step ABI
  // The reference's native boundary hands every step's logits to the host and reorders
  // the self-KV cache when the host asks (decoder256Predict coreml.mm:279-327,
  // decoder1Predict :404-444, rearrange_mkv :251-277), so its Python DecodingTask keeps
  // filters and beam search (decoding.py:707-737).  These entry points serve that
  // caller: the same decoder step as the graph body, without the device token selection.
  int step_prefill(int n_win, int G, const int* init, const int* n_init, int max_init, const int* sot_index,
                   float* lg) override {
    TRY(tm.mark(0, st));
    TRY(begin_batch(n_win, G, init, n_init, max_init, sot_index, -1));
    step_api = true;
    if (lg) HIPCHK(hipMemcpyAsync(lg, logits2, (size_t)2 * n_win * V * 4, hipMemcpyDeviceToHost, st));
    return tm.finish(st, stats[WH_STAT_PREFILL_MS], __func__);
  }

  int step_tokens(const int* tok, const int* offsets, float* lg) override {
    TRY(step_check(tok, offsets));
    const int R = cur_nwin * cur_G;
    TRY(tm.mark(0, st));
    HIPCHK(hipMemcpyAsync(rows_in, tok, R * 4, hipMemcpyHostToDevice, st));
    launch_append_tokens(S, rows_in, cur_nwin, st);
    launch_embed<T>(E, Pdec, ns, nullptr, row_pos, S.hist, S.len, cur_G, HCTX, CTX - 1, x_d, R, st);
    TRY(dec_layers(R, st_row_win, st_row_slot, row_pos, cur_G, cur_nwin, st_win_row0, st_win_nrows, st_win_slot,
                   nullptr, nullptr, 0, true));
    TRY(vocab(nullptr, R, logits));
    if (lg) HIPCHK(hipMemcpyAsync(lg, logits, (size_t)R * V * 4, hipMemcpyDeviceToHost, st));
    TRY(tm.finish(st, stats[WH_STAT_STEPS_MS], __func__));  // the wait: the host tokens outlive their copy
    for (auto& l : h_len) ++l;
    stats[WH_STAT_STEPS] += 1;
    return 0;
  }

  // WHISPER_HIP_XQ=0 keeps the separate cross-query reduce (A/B switch)
  const bool xq_fused = [] {
    const char* e = tune_env("WHISPER_HIP_XQ");
    return !(e && e[0] == '0');
  }();
  // the step's cross-attention query projected inside k_xattn_seg (no cross-q
  // k_proj launch) wherever xattn_fused_q serves the shape; WHISPER_HIP_XQP=0 keeps the
  // split-K projection + slabs (A/B switch)
  static bool xq_proj_on() {
    static const bool on = [] {
      const char* e = tune_env("WHISPER_HIP_XQP");
      return !(e && e[0] == '0');
    }();
    return on;
  }
  bool xq_proj_active(int rows_per_window) const {
    return xq_proj_on() && xattn_fused_q(ns, rows_per_window, (int)sizeof(T));
  }
  int align_rows(const RowPlan& p, const std::vector<int>& sel, float* d_qk, float* d_lg, int eot, const int* ptok,
                 float* probs) override {
    TRY(run_rows(p, 1, d_qk, qk_map, p.R, fp_anc));
    // probabilities of the text tokens, 128 logit rows at a time
    for (int c0 = 0; c0 < (int)sel.size(); c0 += 128) {
      const int rr = std::min<int>(128, (int)sel.size() - c0);
      HIPCHK(hipMemcpyAsync(rows_in, sel.data() + c0, rr * 4, hipMemcpyHostToDevice, st));
      TRY(vocab(rows_in, rr, d_lg));
      launch_token_probs(d_lg, V, rr, eot, ptok + c0, probs + c0, st);
    }
    return 0;
  }

  int score_launch(const T* X, const int* sel, int n, const ScoreOut& o) {
    ScoreArgs a;
    a.X = X; a.E = E; a.x_rows = sel; a.target = o.target; a.rec = (float4_t*)o.rec;
    a.logprob = o.logprob; a.top_id = o.top_id; a.top_logprob = o.top_logprob;
    a.ldx = ns; a.R = n; a.V = V; a.K = ns;
    if (launch_vocab_score<T>(a, st)) return fail(-15, "score: k_score_part does not serve this n_state / n_vocab");
    return 0;
  }
  int score_rows(const RowPlan& p, const int* sel, int n_sel, const ScoreOut& o) override {
    TRY(run_rows(p, 1, nullptr, nullptr, 0, fp_anc));
    return score_launch(xn_d, sel, n_sel, o);
  }
  int score_host_rows(const float* xf, void* xt, int n, const ScoreOut& o) override {
    launch_score_cast<T>(xf, (T*)xt, (int64_t)n * ns, st);
    return score_launch((const T*)xt, nullptr, n, o);
  }

  // Whisper.forward (model.py:110-119): all-row logits of a first pass of `n` tokens at
  // offset 0 for one window slot (beam slot 0, a 1-beam anc layout), optional raw cross-QK of
  // the alignment heads [na][n][1500].  Refused on a slot that is still decoding
  // (check_slot_idle).  The device outputs are carved from the loop's scratch, which no
  // kernel of the first pass touches (its buffers are the activation arena's) and which
  // alignment only uses in calls of its own, before or after this one on the same stream.
  int prefill_logits(int slot, const int* tokens, int n, float* lg, const int* ah, int na, float* aqk) override {
    const size_t b_out = ((size_t)n * V * 4 + 255) & ~size_t(255), b_qk = na > 0 && aqk ? (size_t)na * n * 1500 * 4 : 0;
    TRY(ensure_scratch(b_out + b_qk));
    float* out = (float*)scratch.p;
    float* d_aqk = b_qk ? (float*)(scratch.p + b_out) : nullptr;
    if (!finalized) return fail(-9, "weights not finalized");
    if (slot < 0 || slot >= Wcap || n < 1 || n > CTX) return fail(-15, "bad slot or token count");
    TRY(check_slot_idle(slot));
    for (int i = 0; i < n; ++i)
      if (tokens[i] < 0 || tokens[i] >= V) return fail(-15, "token out of vocabulary");
    // the host vectors of this frame outlive the async copies (the synchronises below)
    RowPlan rows;
    rows.add(slot, slot, tokens, n);
    std::vector<int> map((size_t)Ld * nh, -1), s2(n);
    for (int i = 0; i < na; ++i)
      if (ah[i] >= 0 && ah[i] < Ld * nh) map[ah[i]] = i;
    for (int i = 0; i < n; ++i) s2[i] = i;
    HIPCHK(hipMemcpyAsync(qk_map, map.data(), map.size() * 4, hipMemcpyHostToDevice, st));
    // its own all-zero ancestry table: the decode's S.anc ([w][G][CTX]) stays untouched,
    // so a device-loop decode of other slots can continue afterwards
    TRY(run_rows(rows, 1, d_aqk, d_aqk ? qk_map : nullptr, n, fp_anc));
    for (int r0 = 0; r0 < n; r0 += 128) {
      const int rr = std::min(128, n - r0);
      HIPCHK(hipMemcpyAsync(rows_in, s2.data() + r0, rr * 4, hipMemcpyHostToDevice, st));
      TRY(vocab(rows_in, rr, out + (size_t)r0 * V));
      HIPCHK(hipStreamSynchronize(st));
    }
    HIPCHK(hipMemcpyAsync(lg, out, (size_t)n * V * 4, hipMemcpyDeviceToHost, st));
    if (d_aqk) HIPCHK(hipMemcpyAsync(aqk, d_aqk, (size_t)na * n * 1500 * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    TRY(launch_status(__func__));
    return 0;
  }

  int time_stage(int what, int iters, double* ms) override {
    // the stages run on the live batch's step rows: restore them first (a first pass may
    // have left its own positions in row_pos, where the projections' QKV epilogue would
    // write the decode's self-KV); stages other than whole steps leave x_d dirty
    restore_rows();
    if (what != 0 && what != 7) rows_dirty = true;
    if (what == 0) {
      if (cur_nwin < 1) return fail(-16, "no decode batch");
      if (!eager()) TRY(ensure_graph());
      HIPCHK(hipEventRecord(tm.ev[0], st));
      for (int i = 0; i < iters; ++i) TRY(launch_step());
      HIPCHK(hipEventRecord(tm.ev[1], st));
    } else if (what == 1) {
      HIPCHK(hipEventRecord(tm.ev[0], st));
      for (int i = 0; i < iters; ++i) TRY(encode_chunk(0, 1, true));
      HIPCHK(hipEventRecord(tm.ev[1], st));
    } else if (what == 2 || what == 3 || what == 5 || what == 6) {
      // per-launch time of one decoder-step kernel at the current batch, over all
      // layers (so weights / cross-KV stream from HBM as in the step, not from cache):
      // 2 = the six split-K projection GEMVs of each layer (k_gemv_x, EPI_PARTIAL),
      // 3 = the step's cross-attention (k_xattn_seg)
      // 5 / 6 = 2 / 3 on layer 0 only, repeated (operands Infinity-Cache warm)
      if (cur_nwin < 1) return fail(-16, "no decode batch");
      const bool warm = what >= 5;
      if (warm) what -= 3;
      const int nl = warm ? 1 : Ld;
      const int R = cur_nwin * cur_G, n = ns;
      int launches = 0;
      HIPCHK(hipEventRecord(tm.ev[0], st));
      for (int i = 0; i < iters * (warm ? Ld : 1); ++i)
        for (int l = 0; l < nl; ++l) {
          auto& e = dec[l];
          if (what == 2) {
            TRY(layer_projections(l, R));
            launches += 6;
          } else {
            const T* ck = ckv + (size_t)(2 * l) * Wcap * TKP * n;
            const T* cv = ckv + (size_t)(2 * l + 1) * Wcap * TKP * n;
            XQPart xq = step_xq(cur_G);  // the step's kernel (k_xattn_seg), query from q_d
            if (!p1_active(R, cur_nwin) && xq_proj_active(cur_G)) {
              // or projected in the kernel from xn_d (as the step does)
              xq.qx = xn_d; xq.qwf = e.wqx_f; xq.bias = e.bqx;
            }
            launch_cross_attn<T>(q_d, n, ck, cv, 1500, nh, NSPLIT, cur_nwin, st_win_row0, st_win_nrows, st_win_slot,
                                 (int64_t)TKP * n, po, pm, pl, att_d, n, R, nullptr, nullptr, 0, st, xq, kv8_layer(l));
            ++launches;
          }
        }
      HIPCHK(hipEventRecord(tm.ev[1], st));
      HIPCHK(hipStreamSynchronize(st));
      float t = 0;
      HIPCHK(hipEventElapsedTime(&t, tm.ev[0], tm.ev[1]));
      *ms = t / launches;
      return 0;
    } else if (what == 7) {
      // per-launch time of the step's k_proj projections inside eager steps: every
      // launch carries its own start/stop events (hipExtLaunchKernelGGL: timestamps of
      // the dispatch itself, no marker packets), in the step's kernel order, so each
      // one runs behind its real producer as in the graph (not back to back)
      if (cur_nwin < 1) return fail(-16, "no decode batch");
      const int per_step = 6 * Ld;
      proj_ev.resize(2 * per_step * iters);
      // timing-only events: no system-scope fence (its L2 writeback / invalidate would be
      // charged to the timed kernel; rocprofv3's kernel trace has none)
      for (auto& ev : proj_ev) HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableSystemFence));
      double tot = 0;
      int launches = 0, rc = 0;
      // steps queued back to back as in decode_steps (no host sync between them)
      proj_ev_n = 0;
      for (int i = 0; i < iters && rc == 0; ++i) rc = step_body();
      if (rc == 0 && hipStreamSynchronize(st) != hipSuccess) rc = fail(-100, "time_stage(7): sync failed");
      for (int j = 0; rc == 0 && j < proj_ev_n; ++j) {
        float t = 0;
        if (hipEventElapsedTime(&t, proj_ev[2 * j], proj_ev[2 * j + 1]) != hipSuccess)
          rc = fail(-100, "time_stage(7): hipEventElapsedTime failed");
        tot += t;
        ++launches;
      }
      for (auto& ev : proj_ev)
        if (hipEventDestroy(ev) != hipSuccess && rc == 0) rc = fail(-100, "time_stage(7): hipEventDestroy failed");
      proj_ev.clear();
      proj_ev_n = 0;
      if (rc) return rc;
      *ms = launches ? tot / launches : 0.0;
      return 0;
    } else if (what == 8 || what == 9) {
      // the step's self-attention alone (k_self_attn_qkv, every layer, the live batch at its
      // current context; it rewrites each row's K/V at its next position from the slabs as
      // they stand, which the next real step overwrites): 8 = the decode's ancestry, 9 = every
      // row reading beam slot 0's rows (all beams share one history: the bytes an L2 that
      // deduplicated shared rows perfectly would fetch).  Per-launch ms.
      if (cur_nwin < 1 || cur_G < 1) return fail(-16, "no decode batch");
      if (p1_active(cur_nwin * cur_G, cur_nwin)) return fail(-2, "time_stage(8/9): the single-window step has no k_self_attn_qkv");
      const int R = cur_nwin * cur_G, n = ns;
      const size_t ab = (size_t)Wcap * Gcap * CTX * sizeof(int);
      int* saved = nullptr;
      if (what == 9) {
        HIPCHK(hipMalloc((void**)&saved, ab));
        HIPCHK(hipMemcpyAsync(saved, S.anc, ab, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemsetAsync(S.anc, 0, ab, st));
      }
      int rc = 0;
      if (hipEventRecord(tm.ev[0], st) != hipSuccess) rc = fail(-100, "time_stage(8/9): hipEventRecord failed");
      for (int i = 0; rc == 0 && i < iters; ++i)
        for (int l = 0; rc == 0 && l < Ld; ++l)
          if (launch_self_attn_qkv<T>(part, sa_probe_ks, (int64_t)R * 3 * n, dec[l].bqkv, n, kc[l], vc[l], st_row_win,
                                      st_row_slot, row_pos, S.anc, cur_G, Gcap, nh, CTX, att_d, n, R, st, sa_probe_half))
            rc = fail(-20, "time_stage(8/9): self-attention launch refused");
      if (rc == 0 && hipEventRecord(tm.ev[1], st) != hipSuccess) rc = fail(-100, "time_stage(8/9): hipEventRecord failed");
      if (saved) {
        if (hipMemcpyAsync(S.anc, saved, ab, hipMemcpyDeviceToDevice, st) != hipSuccess && rc == 0)
          rc = fail(-100, "time_stage(9): ancestry restore failed");
        if (hipStreamSynchronize(st) != hipSuccess && rc == 0) rc = fail(-100, "time_stage(9): sync failed");
        if (hipFree(saved) != hipSuccess && rc == 0) rc = fail(-100, "time_stage(9): hipFree failed");
      }
      if (rc) return rc;
      HIPCHK(hipStreamSynchronize(st));
      float t = 0;
      HIPCHK(hipEventElapsedTime(&t, tm.ev[0], tm.ev[1]));
      *ms = t / (iters * Ld);
      return 0;
    } else if (what == 10) {
      // the step's vocabulary projection alone, back to back, on the current batch's rows
      // (the single-window step: the final LayerNorm in its prologue, as after dec_layers_p1)
      if (cur_nwin < 1) return fail(-16, "no decode batch");
      const int R = cur_nwin * cur_G;
      HIPCHK(hipEventRecord(tm.ev[0], st));
      for (int i = 0; i < iters; ++i) {
        final_x = p1_active(R, cur_nwin) ? x_d : nullptr;
        const int rc = vocab(nullptr, R, logits);
        final_x = nullptr;
        if (rc) return rc;
      }
      HIPCHK(hipEventRecord(tm.ev[1], st));
    } else if (what == 4) {
      // the token-selection kernel alone on the current logits (state unchanged)
      if (cur_nwin < 1) return fail(-16, "no decode batch");
      HIPCHK(hipEventRecord(tm.ev[0], st));
      for (int i = 0; i < iters; ++i) launch_logit_rows(logits, V, S, O, cur_nwin, st);
      HIPCHK(hipEventRecord(tm.ev[1], st));
    } else {
      return fail(-2, "time_stage: unknown stage");
    }
    HIPCHK(hipStreamSynchronize(st));
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, tm.ev[0], tm.ev[1]));
    *ms = t / iters;
    return 0;
  }
};

template <typename T>
int create(int device, const wh_dims& dims, int max_windows, int max_group, wh_ctx** out) {
  auto c = new Ctx<T>();
  const int rc = c->init(device, dims, max_windows, max_group);
  if (rc) { delete c; return rc; }
  *out = c;
  return 0;
}

}  // namespace

// ============================================================ C ABI
extern "C" {

const char* wh_last_error(void) { return wh_error().c_str(); }
// 2: wh_decode_opts.no_repeat_ngram / repetition_penalty, 3: wh_set_phrase_bias
int wh_version(void) { return 3; }

int wh_create(int device, const wh_dims* dims, int compute_dtype, int max_windows, int max_group, wh_ctx** out) {
  if (!dims || !out) return fail(-1, "null argument");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(-1, "no HIP device");
  if (device < 0 || device >= ndev) return fail(-1, "device out of range");
  if (compute_dtype == WH_F16) return create<half_t>(device, *dims, max_windows, max_group, out);
  if (compute_dtype == WH_F32) return create<float>(device, *dims, max_windows, max_group, out);
  return fail(-1, "compute_dtype must be WH_F32 or WH_F16");
}

int wh_destroy(wh_ctx* ctx) {
  if (!ctx) return 0;
  if (ctx->sharers > 0)
    return fail(-1, "wh_destroy: " + std::to_string(ctx->sharers) +
                        " context(s) still read this context's weights (wh_tune_share_weights): destroy them first");
  if (ctx->shares_from) --ctx->shares_from->sharers;
  hipSetDevice(ctx->device);
  g_release_error.clear();
  delete ctx;
  if (!g_release_error.empty()) return fail(-100, "wh_destroy: " + g_release_error);
  return 0;
}

// every context call: on the context's device, and no HIP error pending from before it
// (a pending one belongs to an earlier call: reported as such, not as this call's failure)
static int enter(wh_ctx* ctx, const char* entry) {
  if (!ctx) return fail(-1, "null context");
  const hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return fail(-100, std::string(entry) + ": hipSetDevice: " + hipGetErrorString(e));
  const int rc = launch_status("HIP error pending before this call");
  if (rc) wh_error() = std::string(entry) + ": " + wh_error();
  return rc;
}
#define CTXCALL(expr)                            \
  do {                                           \
    const int rc_e = enter(ctx, __func__);       \
    if (rc_e) return rc_e;                       \
    return (expr);                               \
  } while (0)

int wh_set_mel_filters(wh_ctx* ctx, int n_mels, const float* filters) {
  if (!ctx || !filters) return fail(-1, "null argument");
  CTXCALL(ctx->audio.set_mel_filters(n_mels, filters));
}
int wh_set_phrase_bias(wh_ctx* ctx, int n_phrases, const int* tokens, const int* offsets, const float* boost,
                       float start) {
  if (!ctx) return fail(-1, "null context");
  // host state only: no device call, so a decode in progress is not disturbed.  Every check
  // comes before the first write: a refused call leaves the previous table in place
  if (n_phrases == 0) { ctx->bias_tab.clear(); return 0; }
  if (n_phrases < 0 || n_phrases > wh::BIAS_MAX_PHRASES)
    return fail(-11, "phrase_bias: " + std::to_string(n_phrases) + " phrases (0.." + std::to_string(wh::BIAS_MAX_PHRASES) + ")");
  if (!tokens || !offsets || !boost) return fail(-1, "phrase_bias: null argument with n_phrases > 0");
  if (!(start >= 0.f && start <= 1.f)) return fail(-11, "phrase_bias: start must lie in [0, 1]");
  if (offsets[0] != 0) return fail(-11, "phrase_bias: phrase 0: offsets must start at 0");
  std::vector<wh::BiasRec> tab;
  for (int j = 0; j < n_phrases; ++j) {
    const std::string ph = "phrase_bias: phrase " + std::to_string(j);
    // compared before subtracting: hostile offsets must not overflow
    if (offsets[j + 1] <= offsets[j]) return fail(-11, ph + ": offsets must increase (1 to 16 tokens per phrase)");
    if (offsets[j + 1] > offsets[j] + wh::BIAS_MAX_LEN)
      return fail(-11, ph + " is longer than " + std::to_string(wh::BIAS_MAX_LEN) + " tokens");
    if (offsets[j + 1] > wh::BIAS_MAX_ENTRIES)
      return fail(-11, ph + ": more than " + std::to_string(wh::BIAS_MAX_ENTRIES) + " tokens in total");
    if (!(boost[j] > 0.f) || std::isinf(boost[j])) return fail(-11, ph + ": boost must be finite and greater than 0");
    for (int i = offsets[j]; i < offsets[j + 1]; ++i) {
      if (tokens[i] < 0 || tokens[i] >= ctx->V)
        return fail(-11, ph + ": id " + std::to_string(tokens[i]) + " outside the vocabulary [0, " +
                             std::to_string(ctx->V) + ")");
      const int k = i - offsets[j];
      const float start_bonus = boost[j] * start;  // fl32(b * start): one fp32 multiply
      tab.push_back({tokens[i], k, k == 0 ? start_bonus : boost[j], 0});
    }
  }
  ctx->bias_tab.swap(tab);
  return 0;
}
int wh_load_tensor(wh_ctx* ctx, const char* name, const float* data, const int64_t* shape, int ndim) {
  if (!name || !data || !shape) return fail(-1, "null argument");
  CTXCALL(ctx->load(name, data, shape, ndim));
}
int wh_finalize(wh_ctx* ctx) { CTXCALL(ctx->finalize()); }
int wh_token_ms(wh_ctx* ctx, float* out, int cap, int* n, int reset) {
  if (!ctx) return -1;
  const int cnt = (int)ctx->token_ms.size();
  if (n) *n = cnt;
  if (out)
    for (int i = 0; i < cnt && i < cap; ++i) out[i] = ctx->token_ms[i];
  if (reset) ctx->token_ms.clear();
  return 0;
}
int wh_log_mel(wh_ctx* ctx, const float* audio, int64_t n, int64_t pad, int n_mels, int normalize, int64_t* nf) {
  CTXCALL(ctx->audio.log_mel(audio, n, pad, n_mels, normalize, nf));
}
int wh_log_mel_frames(wh_ctx* ctx, const float* audio, int64_t n, int64_t pad, int n_mels, int64_t frame0,
                      int64_t count, int normalize, int64_t* total_frames) {
  CTXCALL(ctx->audio.log_mel_frames(audio, n, pad, n_mels, frame0, count, normalize, total_frames));
}
int wh_audio_upload(wh_ctx* ctx, const float* audio, int64_t n) {
  if (!audio || n <= 0) return fail(-1, "bad audio");
  CTXCALL(ctx->audio.audio_upload(audio, n));
}
int wh_audio_ingest(wh_ctx* ctx, const void* pcm, int format, int64_t n_frames, int channels, int bits, int up,
                    int down, const double* taps, int n_taps, int64_t dst_offset, int64_t reserve, int64_t* n_out) {
  CTXCALL(ctx->audio.audio_ingest(pcm, format, n_frames, channels, bits, up, down, taps, n_taps, dst_offset, reserve, n_out));
}
int wh_audio_read(wh_ctx* ctx, float* out, int64_t offset, int64_t n) { CTXCALL(ctx->audio.audio_read(out, offset, n)); }
int wh_flac_decode_device(wh_ctx* ctx, const uint8_t* data, int64_t n_bytes, int32_t* out, int64_t cap_frames,
                          int64_t* n_frames, int* path_out) {
  CTXCALL(ctx->audio.flac_decode_device(data, n_bytes, out, cap_frames, n_frames, path_out));
}
int wh_flac_ingest(wh_ctx* ctx, const uint8_t* data, int64_t n_bytes, int up, int down, const double* taps, int n_taps,
                   int64_t dst_offset, int64_t reserve, int64_t* n_out, int* path_out) {
  CTXCALL(ctx->audio.flac_ingest(data, n_bytes, up, down, taps, n_taps, dst_offset, reserve, n_out, path_out));
}
int wh_wav_ingest(wh_ctx* ctx, const uint8_t* data, int64_t n_bytes, int up, int down, const double* taps, int n_taps,
                  int64_t dst_offset, int64_t reserve, int64_t* n_out) {
  CTXCALL(ctx->audio.wav_ingest(data, n_bytes, up, down, taps, n_taps, dst_offset, reserve, n_out));
}
int wh_audio_ingest_split(wh_ctx* ctx, const void* pcm, int format, int64_t n_frames, int channels, int bits, int up,
                          int down, const double* taps, int n_taps, const int* select, int n_select,
                          int64_t dst_offset, int64_t reserve, int64_t* n_out) {
  CTXCALL(ctx->audio.audio_ingest_split(pcm, format, n_frames, channels, bits, up, down, taps, n_taps, select, n_select,
                                        dst_offset, reserve, n_out));
}
int wh_flac_ingest_split(wh_ctx* ctx, const uint8_t* data, int64_t n_bytes, int up, int down, const double* taps,
                         int n_taps, const int* select, int n_select, int64_t dst_offset, int64_t reserve,
                         int64_t* n_out, int* path_out) {
  CTXCALL(ctx->audio.flac_ingest_split(data, n_bytes, up, down, taps, n_taps, select, n_select, dst_offset, reserve,
                                       n_out, path_out));
}
int wh_wav_ingest_split(wh_ctx* ctx, const uint8_t* data, int64_t n_bytes, int up, int down, const double* taps,
                        int n_taps, const int* select, int n_select, int64_t dst_offset, int64_t reserve,
                        int64_t* n_out) {
  CTXCALL(ctx->audio.wav_ingest_split(data, n_bytes, up, down, taps, n_taps, select, n_select, dst_offset, reserve,
                                      n_out));
}
int wh_stream_begin(wh_ctx* ctx, int encoding, int channels, int up, int down, const double* taps, int n_taps,
                    int64_t reserve) {
  CTXCALL(ctx->audio.stream_begin(encoding, channels, up, down, taps, n_taps, reserve));
}
int wh_stream_append(wh_ctx* ctx, const void* data, int64_t n_frames, int64_t* n_out) {
  CTXCALL(ctx->audio.stream_append(data, n_frames, n_out));
}
int wh_stream_finish(wh_ctx* ctx, int64_t* n_out) { CTXCALL(ctx->audio.stream_finish(n_out)); }
int wh_stream_trim(wh_ctx* ctx, int64_t n_drop) { CTXCALL(ctx->audio.stream_trim(n_drop)); }
int wh_stream_info(wh_ctx* ctx, int64_t* frames_in, int64_t* samples_out, int64_t* samples_dropped, int* finished) {
  CTXCALL(ctx->audio.stream_info(frames_in, samples_out, samples_dropped, finished));
}
int wh_pool_create(wh_ctx* ctx, int n_slots, int64_t slot_samples) { CTXCALL(ctx->audio.pool_create(n_slots, slot_samples)); }
int wh_pool_destroy(wh_ctx* ctx) { CTXCALL(ctx->audio.pool_destroy()); }
int wh_pool_open(wh_ctx* ctx, int slot, int encoding, int channels, int up, int down, const double* taps, int n_taps) {
  CTXCALL(ctx->audio.pool_open(slot, encoding, channels, up, down, taps, n_taps));
}
int wh_pool_close(wh_ctx* ctx, int slot) { CTXCALL(ctx->audio.pool_close(slot)); }
int wh_pool_append(wh_ctx* ctx, int n, const int* slots, const void* const* data, const int64_t* n_frames,
                   int64_t* n_out) {
  CTXCALL(ctx->audio.pool_append(n, slots, data, n_frames, n_out));
}
int wh_pool_finish(wh_ctx* ctx, int n, const int* slots, int64_t* n_out) { CTXCALL(ctx->audio.pool_finish(n, slots, n_out)); }
int wh_pool_trim(wh_ctx* ctx, int n, const int* slots, const int64_t* n_drop) { CTXCALL(ctx->audio.pool_trim(n, slots, n_drop)); }
int wh_pool_info(wh_ctx* ctx, int slot, int64_t* frames_in, int64_t* samples_out, int64_t* samples_dropped,
                 int* finished) {
  CTXCALL(ctx->audio.pool_info(slot, frames_in, samples_out, samples_dropped, finished));
}
int wh_pool_read(wh_ctx* ctx, int slot, float* out, int64_t offset, int64_t n) {
  CTXCALL(ctx->audio.pool_read(slot, out, offset, n));
}
int wh_pool_log_mel(wh_ctx* ctx, int n, const int* slots, int64_t padding, int n_mels, int64_t* frame_base) {
  CTXCALL(ctx->audio.pool_log_mel(n, slots, padding, n_mels, frame_base));
}
int wh_pool_vad_enable(wh_ctx* ctx, int slot, const wh_svad_opts* opts) { CTXCALL(ctx->audio.pool_vad_enable(slot, opts)); }
int wh_pool_vad_state(wh_ctx* ctx, int n, const int* slots, wh_svad_state* out) { CTXCALL(ctx->audio.pool_vad_state(n, slots, out)); }
int wh_pool_vad_read(wh_ctx* ctx, int slot, uint8_t* ring, int cap, uint32_t* hist) {
  CTXCALL(ctx->audio.pool_vad_read(slot, ring, cap, hist));
}
int wh_stream_vad_enable(wh_ctx* ctx, const wh_svad_opts* opts) { CTXCALL(ctx->audio.stream_vad_enable(opts)); }
int wh_stream_vad_state(wh_ctx* ctx, wh_svad_state* out) { CTXCALL(ctx->audio.stream_vad_state(out)); }
int wh_speech_spans(wh_ctx* ctx, const wh_vad_opts* opts, int n_files, int32_t* spans, int cap, int32_t* n_spans,
                    uint64_t* thresholds) {
  CTXCALL(ctx->audio.speech_spans(opts, n_files, spans, cap, n_spans, thresholds));
}
int wh_frame_energy_read(wh_ctx* ctx, int file, uint64_t* energy_out, int64_t cap, uint32_t* hist_out) {
  CTXCALL(ctx->audio.frame_energy_read(file, energy_out, cap, hist_out));
}
int wh_mel_max(wh_ctx* ctx, float* g) { CTXCALL(ctx->audio.mel_max(g)); }
int wh_log_mel_batch(wh_ctx* ctx, const float* audio, int n_files, const int64_t* n_samples, int64_t pad, int n_mels,
                     int64_t* frame_base) {
  CTXCALL(ctx->audio.log_mel_batch(audio, n_files, n_samples, pad, n_mels, frame_base));
}
int wh_mel_max_batch(wh_ctx* ctx, float* g, int n_files) { CTXCALL(ctx->audio.mel_max_batch(g, n_files)); }
int wh_mel_normalize(wh_ctx* ctx, float g) { CTXCALL(ctx->audio.mel_normalize(g)); }
int wh_mel_read(wh_ctx* ctx, float* out, int64_t f0, int64_t nf) { CTXCALL(ctx->audio.mel_read(out, f0, nf)); }
int wh_mel_write(wh_ctx* ctx, const float* mel, int64_t nf) { CTXCALL(ctx->audio.mel_write(mel, nf, ctx->n_mels)); }
int wh_encode(wh_ctx* ctx, int n_win, const int64_t* seeks, const int* segs) { CTXCALL(ctx->encode(n_win, seeks, segs)); }
int wh_read_audio_features(wh_ctx* ctx, int slot, float* out) { CTXCALL(ctx->read_xa(slot, out)); }
int wh_read_cross_kv(wh_ctx* ctx, int slot, int layer, float* k, float* v) { CTXCALL(ctx->read_ckv(slot, layer, k, v)); }
int wh_set_cross_kv_format(wh_ctx* ctx, int fmt) { CTXCALL(ctx->set_ckv_format(fmt)); }
int wh_set_encoder_format(wh_ctx* ctx, int fmt) { CTXCALL(ctx->set_enc_format(fmt)); }
int wh_set_decoder_format(wh_ctx* ctx, int fmt) { CTXCALL(ctx->set_dec_format(fmt)); }
int wh_read_decoder_w8(wh_ctx* ctx, int layer, int which, uint8_t* codes, float* scales) {
  if (!codes || !scales) return fail(-1, "null argument");
  CTXCALL(ctx->read_dec_w8(layer, which, codes, scales));
}
int wh_set_vocab_format(wh_ctx* ctx, int fmt) { CTXCALL(ctx->set_vocab_format(fmt)); }
int wh_read_vocab_w8(wh_ctx* ctx, uint8_t* codes, float* scales) {
  if (!codes || !scales) return fail(-1, "null argument");
  CTXCALL(ctx->read_vocab_w8(codes, scales));
}
int wh_encoder_kernels(wh_ctx* ctx, int n_win, char* buf, int cap) {
  if (!ctx || !buf || cap < 1) return fail(-1, "bad arguments");
  const std::string d = ctx->encoder_kernels(n_win);
  const int n = std::min<int>((int)d.size(), cap - 1);
  memcpy(buf, d.data(), n);
  buf[n] = 0;
  return n;
}
int wh_fp8_linear(wh_ctx* ctx, int M, int N, int K, const float* x, const float* w, const float* bias, int gelu,
                  int tile, float* y, uint8_t* x_codes, float* x_scales, uint8_t* w_codes, float* w_scales) {
  CTXCALL(ctx->fp8_linear(M, N, K, x, w, bias, gelu, tile, y, x_codes, x_scales, w_codes, w_scales));
}
int wh_read_cross_kv8(wh_ctx* ctx, int slot, int layer, uint8_t* k_codes, float* k_scales, uint8_t* v_codes,
                      float* v_scales) {
  if (!k_codes || !k_scales || !v_codes || !v_scales) return fail(-1, "null argument");
  CTXCALL(ctx->read_ckv8(slot, layer, k_codes, k_scales, v_codes, v_scales));
}
int wh_decode_begin(wh_ctx* ctx, int n_win, const wh_decode_opts* o, const int* init, const int* n_init, int max_init,
                    const int* sot_index) {
  if (!o || !init || !n_init || !sot_index) return fail(-1, "null argument");
  CTXCALL(ctx->decode_begin(n_win, o, init, n_init, max_init, sot_index, nullptr));
}
int wh_decode_begin_slots(wh_ctx* ctx, int n_win, const int* slots, const wh_decode_opts* o, const int* init,
                          const int* n_init, int max_init, const int* sot_index) {
  if (!slots || !o || !init || !n_init || !sot_index) return fail(-1, "null argument");
  CTXCALL(ctx->decode_begin(n_win, o, init, n_init, max_init, sot_index, slots));
}
int wh_decode_steps(wh_ctx* ctx, int max_steps, int* n_done) { CTXCALL(ctx->decode_steps(max_steps, n_done)); }
int wh_decode_read(wh_ctx* ctx, int slot, int* tokens, float* slp, int* len, int* fin_n, int* fin_tok, int* fin_len,
                   float* fin_score, float* nsp) {
  CTXCALL(ctx->decode_read(slot, tokens, slp, len, fin_n, fin_tok, fin_len, fin_score, nsp));
}
int wh_decode_maxc(wh_ctx* ctx) { return ctx ? ctx->maxc_stride : -1; }
int wh_prefill(wh_ctx* ctx, int n_win, int group, const int* tokens, const int* n_tokens, int max_tokens,
               const int* sot_index, float* logits) {
  if (!tokens || !n_tokens || !sot_index) return fail(-1, "null argument");
  CTXCALL(ctx->step_prefill(n_win, group, tokens, n_tokens, max_tokens, sot_index, logits));
}
int wh_step(wh_ctx* ctx, const int* tokens, const int* text_offsets, float* logits) {
  if (!tokens) return fail(-1, "null argument");
  CTXCALL(ctx->step_tokens(tokens, text_offsets, logits));
}
int wh_reorder_kv(wh_ctx* ctx, const int* source_rows) {
  if (!source_rows) return fail(-1, "null argument");
  CTXCALL(ctx->reorder_kv(source_rows));
}
int wh_prefill_logits(wh_ctx* ctx, int slot, const int* tokens, int n, float* logits, const int* ah, int na, float* aqk) {
  CTXCALL(ctx->prefill_logits(slot, tokens, n, logits, ah, na, aqk));
}
int wh_align(wh_ctx* ctx, int slot, const int* tokens, int n_tokens, int n_sot, int num_frames, const int* align_heads,
             int n_align, int medfilt_width, float* token_probs, int* path, int* path_len) {
  CTXCALL(ctx->align_windows(1, &slot, tokens, &n_tokens, n_sot, &num_frames, align_heads, n_align, medfilt_width,
                             nullptr, 0.f, token_probs, path, path_len, nullptr));
}
int wh_align_batch(wh_ctx* ctx, int n_win, const int* slots, const int* tokens, const int* n_tokens, int n_sot,
                   const int* num_frames, const int* align_heads, int n_align, int medfilt_width, float* token_probs,
                   int* paths, int* path_lens) {
  CTXCALL(ctx->align_windows(n_win, slots, tokens, n_tokens, n_sot, num_frames, align_heads, n_align, medfilt_width,
                             nullptr, 0.f, token_probs, paths, path_lens, nullptr));
}
int wh_dtw(wh_ctx* ctx, const float* x, int n_rows, int n_cols, int* path, int* path_len) {
  CTXCALL(ctx->dtw(x, n_rows, n_cols, path, path_len, nullptr));
}
int wh_dtw_open(wh_ctx* ctx, const float* x, int n_rows, int n_cols, int min_rows, float row_penalty, int* path,
                int* path_len, int* end_row, float* end_scores) {
  // refused here, before the context is entered (no HIP call yet)
  if (!x || !path || !path_len || !end_row) return fail(-1, "wh_dtw_open: null argument (x, path, path_len or end_row)");
  if (n_rows > 1023) return fail(-15, "wh_dtw_open: n_rows above 1023");
  if (n_rows < 1 || n_cols < 1 || (int64_t)n_rows * n_cols > (int64_t)1 << 26)
    return fail(-15, "wh_dtw_open: n_rows / n_cols out of range");
  if (min_rows < 0 || min_rows > n_rows) return fail(-15, "wh_dtw_open: min_rows outside 0..n_rows");
  if (!(row_penalty >= 0.f) || std::isinf(row_penalty))
    return fail(-15, "wh_dtw_open: row_penalty must be finite and >= 0");
  const DecodeLoop::DtwOpen open{min_rows, row_penalty, end_row, end_scores};
  CTXCALL(ctx->dtw(x, n_rows, n_cols, path, path_len, &open));
}
int wh_align_batch_open(wh_ctx* ctx, int n_win, const int* slots, const int* tokens, const int* n_tokens, int n_sot,
                        const int* num_frames, const int* align_heads, int n_align, int medfilt_width,
                        const int* min_rows, float row_penalty, float* token_probs, int* paths, int* path_lens,
                        int* end_rows) {
  // refused here, before the context is entered (no HIP call yet)
  if (!slots || !tokens || !n_tokens || !num_frames || !align_heads || !min_rows || !token_probs || !paths ||
      !path_lens || !end_rows)
    return fail(-1, "wh_align_batch_open: null argument");
  if (!(row_penalty >= 0.f) || std::isinf(row_penalty))
    return fail(-15, "wh_align_batch_open: row_penalty must be finite and >= 0");
  for (int w = 0; w < n_win; ++w) {
    const int n_rows = n_tokens[w] - n_sot - 1;  // the text tokens and the row that predicts eot
    if (n_rows > 1023) return fail(-15, "wh_align_batch_open: n_rows above 1023 (window " + std::to_string(w) + ")");
    if (min_rows[w] < 0 || min_rows[w] > std::max(n_rows, 0))
      return fail(-15, "wh_align_batch_open: min_rows of window " + std::to_string(w) + " outside 0..n_rows");
  }
  CTXCALL(ctx->align_windows(n_win, slots, tokens, n_tokens, n_sot, num_frames, align_heads, n_align, medfilt_width,
                             min_rows, row_penalty, token_probs, paths, path_lens, end_rows));
}
int wh_vocab_score(wh_ctx* ctx, const float* x, int n_rows, const int* targets, float* logprob, int* top_id,
                   float* top_logprob) {
  // refused here, before the context is entered (no HIP call yet)
  if (!ctx) return fail(-1, "wh_vocab_score: null context");
  const int rc = ctx->vocab_score_check(x, n_rows, targets, logprob, top_id, top_logprob);
  if (rc) return rc;
  CTXCALL(ctx->vocab_score(x, n_rows, targets, logprob, top_id, top_logprob));
}
int wh_score_batch(wh_ctx* ctx, int n_seq, const int* slots, const int* tokens, const int* n_tokens, const int* n_ctx,
                   float* logprob, int* top_id, float* top_logprob) {
  // refused here, before the context is entered (no HIP call yet)
  if (!ctx) return fail(-1, "wh_score_batch: null context");
  const int rc = ctx->score_check(n_seq, slots, tokens, n_tokens, n_ctx, logprob, top_id, top_logprob);
  if (rc) return rc;
  CTXCALL(ctx->score_windows(n_seq, slots, tokens, n_tokens, n_ctx, logprob, top_id, top_logprob));
}
int wh_stats(wh_ctx* ctx, double* out, int n) {
  if (!ctx || !out) return fail(-1, "null argument");
  for (int i = 0; i < n && i < WH_N_STATS; ++i) out[i] = ctx->stats[i];
  return 0;
}
int wh_step_kernels(wh_ctx* ctx, int n_win, int group, char* buf, int cap) {
  if (!ctx || !buf || cap < 1) return fail(-1, "bad arguments");
  const std::string d = ctx->step_kernels(n_win, group);
  const int n = std::min<int>((int)d.size(), cap - 1);
  memcpy(buf, d.data(), n);
  buf[n] = 0;
  return n;
}
int wh_sync(wh_ctx* ctx) {
  const int rc = enter(ctx, __func__);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize());
  return launch_status(__func__);
}
int wh_time_stage(wh_ctx* ctx, int what, int iters, double* ms) { CTXCALL(ctx->time_stage(what, iters, ms)); }
#if WH_TUNING
int wh_tune_share_weights(wh_ctx* ctx, wh_ctx* src) {
  if (!src) return fail(-1, "null source context");
  CTXCALL(ctx->share_weights_from(src));
}
#endif

}  // extern "C"
