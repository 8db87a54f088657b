// What a context keeps in device memory, each thing written down once: the arena that
// measures and carves, the layouts of the weight and the activation / state arena, and the
// tables of the tensors wh_load_tensor takes.  The layouts are templates over the context
// (its element type C::elem and its pointer members), so tools/layout_host_check.cpp runs
// the same code on a stand-in under the host sanitizers.  No HIP in it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <utility>
#include <vector>

namespace wh {

constexpr int PRE_ROWS = 1024;  // min prefill rows per pass (the context sizes it to ~240 per window)
constexpr int MROWS = 3008;     // melT rows per window (1 pad + 3000 + slack for padded conv1 K)
constexpr int H1ROWS = 3002;    // conv1 output rows per window (zero rows 0 and 3001)
constexpr int NSPLIT = 8;       // cross-attention key splits (1500 / 8 = 188 keys)
constexpr int RSPLIT = 16;      // max split-K slabs of the residual projections (decode rows <= 128)
constexpr int KC = 9;
constexpr int P1_SLABS = 2048;  // k_proj1 split-K slabs: zs x 16-column tiles <= 16 x 80 at n = 1280
// 128 x 64 tiles of a single window's n-wide encoder GEMMs (1500 rows: 12 row tiles)
constexpr int EKZ_TILES(int n) { return 12 * (n / 64); }

// Every allocation is its layout's measured size plus this much after the last buffer.
// Nothing is known to read there.
constexpr size_t ARENA_TAIL_PAD = 65536;

// A bump allocator over one device allocation, every buffer 256-aligned.  With no base it
// measures: take advances off as it does when carving and returns a value that must not be
// dereferenced; off is the size afterwards.
struct Arena {
  char* base = nullptr;
  size_t cap = 0, off = 0;
  bool over = false;  // a take went past cap
  std::vector<std::pair<size_t, size_t>>* trace = nullptr;  // (offset, bytes) of every take, for the host check
  Arena() = default;
  Arena(void* b, size_t c) : base((char*)b), cap(c) {}
  void* take_bytes(size_t bytes) {
    off = (off + 255) & ~size_t(255);
    if (trace) trace->push_back({off, bytes});
    void* p = (void*)((uintptr_t)base + off);
    off += bytes;
    if (base && off > cap) over = true;
    return p;
  }
  template <typename U>
  U* take(size_t elems) { return (U*)take_bytes(elems * sizeof(U)); }
  // p + elems without arithmetic on a pointer that a measuring run made up
  template <typename U>
  static U* at(U* p, size_t elems) { return (U*)((uintptr_t)p + elems * sizeof(U)); }
  bool ok() const { return !over; }
};

template <typename T>
struct EncLayer {
  float *ln1_g, *ln1_b, *bqkv, *bo, *ln2_g, *ln2_b, *b1, *b2;
  T *wqkv, *wo, *w1, *w2;
};
// the 8-bit copy of an encoder layer's four weights: codes [out][in], one scale per out
struct Enc8Layer {
  uint8_t *wqkv, *wo, *w1, *w2;
  float *sqkv, *so, *s1, *s2;
};
// a decoder layer: the encoder layer's members and the cross-attention's
template <typename T>
struct DecLayer : EncLayer<T> {
  float *lnx_g, *lnx_b, *bqx, *box;
  T *wqx, *wox;
  // this layer's cross-attention K, V weights [2][n][n] and biases [2][n] inside the
  // context's ckv_w / ckv_b (all layers' cross-KV is one GEMM)
  T* ckw;
  float* ckb;
  // W_q in the in-kernel query projection's fragment order (xq_project: each wave's
  // 16 B-per-lane loads are 1 KB contiguous), fp16 contexts whose shape xattn_fused_q serves
  T* wqx_f = nullptr;
};

// the 8-bit copy of a decoder layer's six linear weights (wh_set_decoder_format), indexed as
// wh_read_decoder_w8's `which`: 0 qkv, 1 o, 2 xq, 3 xo, 4 fc1, 5 fc2.  Codes [out][in] in
// k_proj1<w8>'s fragment order (wh_proj8.h), one scale per out
struct Dec8Layer {
  uint8_t* w[6];
  float* s[6];
};
constexpr size_t DEC8_OUT[6] = {3, 1, 1, 1, 4, 1}, DEC8_IN[6] = {1, 1, 1, 1, 1, 4};  // rows, columns in units of n

// the sizes the layouts and the tensor shapes depend on
struct LayoutDims {
  size_t n, n_mels, K1p, La, Ld, V, nh;  // the model's (K1p: conv1's K, 3 * n_mels padded to 128 B)
  size_t Wcap, Gcap;                     // max_windows, max_group
  size_t WE, RD, LR;                     // encoder windows per pass, decoder rows, logit rows
  bool wq_frag;                          // the fragment-ordered W_q copies exist (xattn_fused_q)
  // of the kernels (wh_kernels.h, wh_loop.h), by value so that this header includes no HIP:
  // TKP, CTX, HCTX, LP_SLICES * LP_REC, XS_NSP * XREC, BIAS_MAX_ENTRIES
  size_t tkp, ctx, hctx, lp_words, xs_words, bias_entries;
};

template <class C>
void layout_weights(C& c, Arena& ar, const LayoutDims& d) {
  using T = typename C::elem;
  const size_t n = d.n;
  auto tk = [&](size_t elems) { return ar.take<T>(elems); };
  auto fk = [&](size_t elems) { return ar.take<float>(elems); };
  c.conv1_w = tk(n * d.K1p); c.conv1_b = fk(n); c.conv2_w = tk(n * 3 * n); c.conv2_b = fk(n); c.pos_enc = fk(1500 * n);
  c.enc.resize(d.La);
  for (auto& e : c.enc) {
    e.ln1_g = fk(n); e.ln1_b = fk(n); e.wqkv = tk(3 * n * n); e.bqkv = fk(3 * n); e.wo = tk(n * n); e.bo = fk(n);
    e.ln2_g = fk(n); e.ln2_b = fk(n); e.w1 = tk(4 * n * n); e.b1 = fk(4 * n); e.w2 = tk(4 * n * n); e.b2 = fk(n);
  }
  c.lnp_g = fk(n); c.lnp_b = fk(n);
  c.E = tk(d.V * n); c.Pdec = tk(d.ctx * n);
  c.dec.resize(d.Ld);
  for (auto& e : c.dec) {
    e.ln1_g = fk(n); e.ln1_b = fk(n); e.wqkv = tk(3 * n * n); e.bqkv = fk(3 * n); e.wo = tk(n * n); e.bo = fk(n);
    e.lnx_g = fk(n); e.lnx_b = fk(n); e.wqx = tk(n * n); e.bqx = fk(n); e.wox = tk(n * n); e.box = fk(n);
    e.ln2_g = fk(n); e.ln2_b = fk(n); e.w1 = tk(4 * n * n); e.b1 = fk(4 * n); e.w2 = tk(4 * n * n); e.b2 = fk(n);
  }
  c.ln_g = fk(n); c.ln_b = fk(n);
  c.ckv_w = tk(2 * d.Ld * n * n); c.ckv_b = fk(2 * d.Ld * n);
  for (size_t l = 0; l < d.Ld; ++l) {
    c.dec[l].ckw = Arena::at(c.ckv_w, 2 * l * n * n);
    c.dec[l].ckb = Arena::at(c.ckv_b, 2 * l * n);
  }
  if (d.wq_frag)
    for (auto& e : c.dec) e.wqx_f = tk(n * n);
}

// the decoder's 8-bit weight copies: an arena of their own, allocated when the format first
// asks for them (the default context allocates what it did before)
template <class C>
void layout_dec8(C& c, Arena& ar, const LayoutDims& d) {
  c.dec8.resize(d.Ld);
  for (auto& q : c.dec8)
    for (int i = 0; i < 6; ++i) {
      q.w[i] = ar.take<uint8_t>(DEC8_OUT[i] * d.n * DEC8_IN[i] * d.n);
      q.s[i] = ar.take<float>(DEC8_OUT[i] * d.n);
    }
}

// activations and decode state
template <class C>
void layout_buffers(C& c, Arena& ar, const LayoutDims& d) {
  using T = typename C::elem;
  const size_t n = d.n, nh = d.nh, V = d.V, WE = d.WE, RD = d.RD, Wcap = d.Wcap, WG = d.Wcap * d.Gcap;
  auto ta = [&](size_t elems) { return ar.take<T>(elems); };
  auto fa = [&](size_t elems) { return ar.take<float>(elems); };
  auto ia = [&](size_t elems) { return ar.take<int>(elems); };
  c.melT = ta(WE * MROWS * d.n_mels); c.h1 = ta(WE * H1ROWS * n);
  c.x_e = fa(WE * 1500 * n); c.xn_e = ta(WE * 1500 * n); c.qkv_e = ta(WE * 1500 * 3 * n);
  c.att_e = ta(WE * 1500 * n); c.hm_e = ta(WE * 1500 * 4 * n);
  c.vt_e = ta(WE * nh * 64 * d.tkp + 64);  // encoder V^T (padding keys stay zero) + the last key tile's read past TKP
  c.xa = ta(Wcap * 1500 * n);
  c.ckv = ta(2 * d.Ld * Wcap * d.tkp * n + 32768 / sizeof(T));  // + 32768 B: the last key tile reads past TKP
  c.kc.resize(d.Ld); c.vc.resize(d.Ld);
  for (size_t l = 0; l < d.Ld; ++l) { c.kc[l] = ta(WG * d.ctx * n); c.vc[l] = ta(WG * d.ctx * n); }
  c.x_d = fa(RD * n); c.xn_d = ta(RD * n); c.q_d = ta(RD * n); c.att_d = ta(RD * n);
  c.hm_d = ta(RD * 4 * n);
  c.po = fa(RD * nh * NSPLIT * 64); c.pm = fa(RD * nh * NSPLIT); c.pl = fa(RD * nh * NSPLIT);
  c.logits = fa(d.LR * V); c.logits2 = fa(2 * Wcap * V); c.nsp = fa(Wcap); c.part = fa(RSPLIT * RD * n);
  c.row_tok = ia(RD); c.row_pos = ia(RD); c.row_win = ia(RD); c.row_slot = ia(RD); c.win_row0 = ia(RD); c.win_nrows = ia(RD);
  c.win_slot = ia(RD); c.rows_in = ia(RD); c.src_rows = ia(RD);
  c.st_row_win = ia(RD); c.st_row_slot = ia(RD); c.st_win_row0 = ia(RD); c.st_win_nrows = ia(RD); c.st_win_slot = ia(RD);
  c.qk_map = ia(d.Ld * nh);
  c.suppress = ar.take<unsigned>((V + 31) / 32);
  c.d_seeks = ar.take<int64_t>(Wcap); c.d_segs = ia(Wcap);
  auto& S = c.S;
  S.hist = ia(WG * d.hctx); S.anc = ia(WG * d.ctx);
  c.fp_anc = ia(Wcap * d.ctx);  // first passes' ancestry: all zero (beam slot 0), never written
  S.len = ia(Wcap); S.sample_begin = ia(Wcap); S.step = ia(Wcap); S.done = ia(Wcap); S.fin_n = ia(Wcap);
  S.sum_lp = fa(WG);
  S.fin_score = fa(Wcap * 16); S.fin_len = ia(Wcap * 16); S.fin_tok = ia(Wcap * 16 * d.hctx);
  S.cand_val = fa(WG * KC); S.cand_idx = ia(WG * KC);
  S.lpart = fa(WG * d.lp_words); S.lp_cnt = ia(WG);  // zeroed with the arena
  S.lpw_cnt = ia(Wcap);  // window arrival counters of the merging selection
  S.seed = ar.take<unsigned long long>(8);
  c.p1_slab = fa((size_t)P1_SLABS * 256); c.p1_cnt = ia(4 * n / 16);  // k_proj1 split-K slabs + counters, zeroed with the arena
  c.xs_rec = fa(Wcap * nh * d.xs_words); c.xs_cnt = ia(Wcap * nh);  // cross-attention segment records
  c.x2_d = fa(8 * n);  // k_proj1 path (<= 8 rows, wh_proj.h P1_RMAX): the second residual buffer
  c.ekz_slab = fa((size_t)EKZ_TILES((int)n) * 16384); c.ekz_cnt = ia((size_t)EKZ_TILES((int)n) * 4);  // single-window encoder K halves, zeroed with the arena
  using Bias = typename std::remove_pointer<decltype(c.bias_dev)>::type;
  c.bias_dev = ar.take<Bias>(d.bias_entries);  // the phrase table, at its capacity
}

// ------------------------------------------------------------ loadable tensors
// One tensor wh_load_tensor takes and where in L (a layer, or the context) it lands.
template <class L, typename T>
struct Tensor {
  const char* name;   // in a block: what follows "encoder.blocks.N." / "decoder.blocks.N."
  const char* shape;  // a letter per dimension: n, f = 4 n, m = n_mels, v = n_vocab, c = text ctx, a = 1500, 3
  T* L::*wt;                  // stored as T in this member, or
  float* L::*wf = nullptr;    // as float in this one,
  int slot = 0;  // at element slot * (the tensor's size): K, V behind Q in wqkv / bqkv, V behind K in ckw / ckb
  float scale[2] = {1.f, 1.f};  // folded in at load, fp32: [0] in an encoder layer or the context, [1] in a decoder layer
};
inline int64_t dim_size(char u, const LayoutDims& d) {
  return int64_t(u == 'n' ? d.n : u == 'f' ? 4 * d.n : u == 'm' ? d.n_mels : u == 'v' ? d.V : u == 'c' ? d.ctx : u == 'a' ? 1500 : 3);
}
constexpr float WH_KS = 0.125f;  // (64)^-0.5: the encoder's keys (encoder.py:38), the decoder's queries (decoder.py:20)

// the 15 tensors of an encoder block, which a decoder block has too
template <typename T>
const std::vector<Tensor<EncLayer<T>, T>>& block_tensors() {
  using E = EncLayer<T>;
  static const std::vector<Tensor<E, T>> t = {
      {"attn.query.weight", "nn", &E::wqkv, nullptr, 0, {1.f, WH_KS}}, {"attn.query.bias", "n", nullptr, &E::bqkv, 0, {1.f, WH_KS}},
      {"attn.key.weight", "nn", &E::wqkv, nullptr, 1, {WH_KS, 1.f}},
      {"attn.value.weight", "nn", &E::wqkv, nullptr, 2}, {"attn.value.bias", "n", nullptr, &E::bqkv, 2},
      {"attn.out.weight", "nn", &E::wo}, {"attn.out.bias", "n", nullptr, &E::bo},
      {"attn_ln.weight", "n", nullptr, &E::ln1_g}, {"attn_ln.bias", "n", nullptr, &E::ln1_b},
      {"mlp_ln.weight", "n", nullptr, &E::ln2_g}, {"mlp_ln.bias", "n", nullptr, &E::ln2_b},
      {"mlp.0.weight", "fn", &E::w1}, {"mlp.0.bias", "f", nullptr, &E::b1},
      {"mlp.2.weight", "nf", &E::w2}, {"mlp.2.bias", "n", nullptr, &E::b2},
  };
  return t;
}
// the 9 more of a decoder block
template <typename T>
const std::vector<Tensor<DecLayer<T>, T>>& cross_tensors() {
  using E = DecLayer<T>;
  static const std::vector<Tensor<E, T>> t = {
      {"cross_attn.query.weight", "nn", &E::wqx, nullptr, 0, {1.f, WH_KS}}, {"cross_attn.query.bias", "n", nullptr, &E::bqx, 0, {1.f, WH_KS}},
      {"cross_attn.key.weight", "nn", &E::ckw},
      {"cross_attn.value.weight", "nn", &E::ckw, nullptr, 1}, {"cross_attn.value.bias", "n", nullptr, &E::ckb, 1},
      {"cross_attn.out.weight", "nn", &E::wox}, {"cross_attn.out.bias", "n", nullptr, &E::box},
      {"cross_attn_ln.weight", "n", nullptr, &E::lnx_g}, {"cross_attn_ln.bias", "n", nullptr, &E::lnx_b},
  };
  return t;
}
// the 11 outside the blocks, by their full names (C: the context).  The convolutions'
// weights [n][c][3] are uploaded tap-major, [n][3][c]
template <class C>
const std::vector<Tensor<C, typename C::elem>>& top_tensors() {
  static const std::vector<Tensor<C, typename C::elem>> t = {
      {"encoder.conv1.weight", "nm3", &C::conv1_w}, {"encoder.conv1.bias", "n", nullptr, &C::conv1_b},
      {"encoder.conv2.weight", "nn3", &C::conv2_w}, {"encoder.conv2.bias", "n", nullptr, &C::conv2_b},
      {"encoder.positional_embedding", "an", nullptr, &C::pos_enc},
      {"encoder.ln_post.weight", "n", nullptr, &C::lnp_g}, {"encoder.ln_post.bias", "n", nullptr, &C::lnp_b},
      {"decoder.token_embedding.weight", "vn", &C::E}, {"decoder.positional_embedding", "cn", &C::Pdec},
      {"decoder.ln.weight", "n", nullptr, &C::ln_g}, {"decoder.ln.bias", "n", nullptr, &C::ln_b},
  };
  return t;
}
// the tensors a model of La + Ld layers needs before wh_finalize
template <class C>
size_t n_loadable(size_t La, size_t Ld) {
  using T = typename C::elem;
  return top_tensors<C>().size() + (La + Ld) * block_tensors<T>().size() + Ld * cross_tensors<T>().size();
}

}  // namespace wh
