// The arena, the two layouts of a context and its tensor tables (csrc/wh_layout.h) under the
// host sanitizers, without a context, a GPU or Python:
//   make -C whisper.coreml_amd tools/layout_host_check && ./whisper.coreml_amd/tools/layout_host_check
// The layouts run on a stand-in for Ctx<T> that has the pointer members and nothing else, for
// the micro model (n 128, 2 + 2 layers, 2 heads, V 51865, 80 mels) with max_windows 2 and
// max_group 5, in both element sizes.  The expected (buffer, bytes) sequences are written out
// by hand from the carving lists of the commit before the layouts existed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "wh_layout.h"

static int failures = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      ++failures;                   \
      fprintf(stderr, "FAIL ");     \
      fprintf(stderr, __VA_ARGS__); \
      fputc('\n', stderr);          \
    }                               \
  } while (0)

template <typename T>
struct Stand {
  using elem = T;
  T *conv1_w, *conv2_w, *E, *Pdec, *ckv_w;
  float *conv1_b, *conv2_b, *pos_enc, *lnp_g, *lnp_b, *ln_g, *ln_b, *ckv_b;
  std::vector<wh::EncLayer<T>> enc;
  std::vector<wh::DecLayer<T>> dec;
  T *melT, *h1, *xn_e, *qkv_e, *vt_e, *att_e, *hm_e, *xa, *ckv, *xn_d, *q_d, *att_d, *hm_d;
  std::vector<T*> kc, vc;
  float *x_e, *x_d, *po, *pm, *pl, *logits, *logits2, *nsp, *part, *p1_slab, *xs_rec, *x2_d, *ekz_slab;
  int *row_tok, *row_pos, *row_win, *row_slot, *win_row0, *win_nrows, *win_slot, *rows_in, *src_rows;
  int *st_row_win, *st_row_slot, *st_win_row0, *st_win_nrows, *st_win_slot;
  int *qk_map, *d_segs, *fp_anc, *p1_cnt, *xs_cnt, *ekz_cnt;
  unsigned* suppress;
  int64_t* d_seeks;
  struct {
    int *hist, *anc, *len, *sample_begin, *step, *done, *fin_n, *fin_len, *fin_tok, *cand_idx, *lp_cnt, *lpw_cnt;
    float *sum_lp, *fin_score, *cand_val, *lpart;
    unsigned long long* seed;
  } S;
  struct Bias { int id, k; float bonus; int pad; }* bias_dev;
};

struct Want {
  const char* name;
  const void* p;
  size_t bytes;
};
using Trace = std::vector<std::pair<size_t, size_t>>;

// measure, carve, and hold the carving against `want` (built from the carved stand-in)
template <class Layout, class WantFn>
static void check_arena(const char* what, Layout layout, WantFn want_of) {
  wh::Arena m;
  layout(m);
  char* base = (char*)aligned_alloc(256, (m.off + 255) & ~size_t(255));
  Trace tr;
  wh::Arena ar(base, m.off);
  ar.trace = &tr;
  layout(ar);
  CHECK(ar.ok(), "%s: overflow at the measured size", what);
  CHECK(ar.off == m.off, "%s: measured %zu bytes, carved %zu", what, m.off, ar.off);
  const std::vector<Want> want = want_of();
  CHECK(tr.size() == want.size(), "%s: %zu buffers, want %zu", what, tr.size(), want.size());
  size_t end = 0;
  for (size_t i = 0; i < tr.size() && i < want.size(); ++i) {
    const size_t off = tr[i].first, bytes = tr[i].second;
    CHECK((const char*)want[i].p == base + off, "%s: buffer %zu is not %s", what, i, want[i].name);
    CHECK(bytes == want[i].bytes, "%s: %s has %zu bytes, want %zu", what, want[i].name, bytes, want[i].bytes);
    CHECK(off % 256 == 0, "%s: %s at offset %zu is not 256-aligned", what, want[i].name, off);
    CHECK(off >= end, "%s: %s at %zu overlaps the buffer before it (ends %zu)", what, want[i].name, off, end);
    end = off + bytes;
    CHECK(end <= ar.cap, "%s: %s ends at %zu, past the capacity %zu", what, want[i].name, end, ar.cap);
  }
  wh::Arena one_short(base, m.off - 1);
  layout(one_short);
  CHECK(!one_short.ok(), "%s: an arena one byte short reports ok", what);
  free(base);
}

template <typename T>
static void check_micro() {
  const size_t e = sizeof(T);
  const char* dt = e == 2 ? "16-bit" : "32-bit";
  wh::LayoutDims d{};
  d.n = 128; d.n_mels = 80; d.K1p = 256; d.La = 2; d.Ld = 2; d.V = 51865; d.nh = 2;
  d.Wcap = 2; d.Gcap = 5; d.WE = 2; d.RD = 1024; d.LR = 10; d.wq_frag = false;
  d.tkp = 1536; d.ctx = 448; d.hctx = 449; d.lp_words = 32 * 32; d.xs_words = 24 * 1056; d.bias_entries = 512;
  Stand<T> c{};

  check_arena(dt, [&](wh::Arena& ar) { wh::layout_weights(c, ar, d); }, [&] {
    std::vector<Want> w = {{"conv1_w", c.conv1_w, 128 * 256 * e}, {"conv1_b", c.conv1_b, 512},
                           {"conv2_w", c.conv2_w, 128 * 384 * e}, {"conv2_b", c.conv2_b, 512},
                           {"pos_enc", c.pos_enc, 1500 * 128 * 4}};
    for (auto& l : c.enc) {
      w.insert(w.end(), {{"enc.ln1_g", l.ln1_g, 512}, {"enc.ln1_b", l.ln1_b, 512}, {"enc.wqkv", l.wqkv, 3 * 16384 * e},
                         {"enc.bqkv", l.bqkv, 1536}, {"enc.wo", l.wo, 16384 * e}, {"enc.bo", l.bo, 512},
                         {"enc.ln2_g", l.ln2_g, 512}, {"enc.ln2_b", l.ln2_b, 512}, {"enc.w1", l.w1, 65536 * e},
                         {"enc.b1", l.b1, 2048}, {"enc.w2", l.w2, 65536 * e}, {"enc.b2", l.b2, 512}});
    }
    w.insert(w.end(), {{"lnp_g", c.lnp_g, 512}, {"lnp_b", c.lnp_b, 512}, {"E", c.E, 51865 * 128 * e},
                       {"Pdec", c.Pdec, 448 * 128 * e}});
    for (auto& l : c.dec) {
      w.insert(w.end(), {{"dec.ln1_g", l.ln1_g, 512}, {"dec.ln1_b", l.ln1_b, 512}, {"dec.wqkv", l.wqkv, 3 * 16384 * e},
                         {"dec.bqkv", l.bqkv, 1536}, {"dec.wo", l.wo, 16384 * e}, {"dec.bo", l.bo, 512},
                         {"dec.lnx_g", l.lnx_g, 512}, {"dec.lnx_b", l.lnx_b, 512}, {"dec.wqx", l.wqx, 16384 * e},
                         {"dec.bqx", l.bqx, 512}, {"dec.wox", l.wox, 16384 * e}, {"dec.box", l.box, 512},
                         {"dec.ln2_g", l.ln2_g, 512}, {"dec.ln2_b", l.ln2_b, 512}, {"dec.w1", l.w1, 65536 * e},
                         {"dec.b1", l.b1, 2048}, {"dec.w2", l.w2, 65536 * e}, {"dec.b2", l.b2, 512}});
    }
    w.insert(w.end(), {{"ln_g", c.ln_g, 512}, {"ln_b", c.ln_b, 512}, {"ckv_w", c.ckv_w, 4 * 16384 * e},
                       {"ckv_b", c.ckv_b, 4 * 512}});
    return w;
  });
  // the cross-KV views of the layers: K then V of layer l at 2 l, 2 l + 1
  for (size_t l = 0; l < 2; ++l) {
    CHECK(c.dec[l].ckw == c.ckv_w + 2 * l * 16384, "%s: layer %zu's ckw", dt, l);
    CHECK(c.dec[l].ckb == c.ckv_b + 2 * l * 128, "%s: layer %zu's ckb", dt, l);
    CHECK(c.dec[l].wqx_f == nullptr, "%s: layer %zu has a W_q copy", dt, l);
  }

  check_arena(dt, [&](wh::Arena& ar) { wh::layout_buffers(c, ar, d); }, [&] {
    const size_t rows = 1024 * 4, win = 2 * 4, kv = 10 * 448 * 128 * e;
    return std::vector<Want>{
        {"melT", c.melT, 2 * 3008 * 80 * e}, {"h1", c.h1, 2 * 3002 * 128 * e}, {"x_e", c.x_e, 2 * 1500 * 128 * 4},
        {"xn_e", c.xn_e, 2 * 1500 * 128 * e}, {"qkv_e", c.qkv_e, 2 * 1500 * 384 * e},
        {"att_e", c.att_e, 2 * 1500 * 128 * e}, {"hm_e", c.hm_e, 2 * 1500 * 512 * e},
        {"vt_e", c.vt_e, (2 * 2 * 64 * 1536 + 64) * e}, {"xa", c.xa, 2 * 1500 * 128 * e},
        {"ckv", c.ckv, 2 * 2 * 2 * 1536 * 128 * e + 32768},
        {"kc[0]", c.kc[0], kv}, {"vc[0]", c.vc[0], kv}, {"kc[1]", c.kc[1], kv}, {"vc[1]", c.vc[1], kv},
        {"x_d", c.x_d, 1024 * 128 * 4}, {"xn_d", c.xn_d, 1024 * 128 * e}, {"q_d", c.q_d, 1024 * 128 * e},
        {"att_d", c.att_d, 1024 * 128 * e}, {"hm_d", c.hm_d, 1024 * 512 * e},
        {"po", c.po, 1024 * 2 * 8 * 64 * 4}, {"pm", c.pm, 1024 * 2 * 8 * 4}, {"pl", c.pl, 1024 * 2 * 8 * 4},
        {"logits", c.logits, 10 * 51865 * 4}, {"logits2", c.logits2, 4 * 51865 * 4}, {"nsp", c.nsp, win},
        {"part", c.part, 16 * 1024 * 128 * 4},
        {"row_tok", c.row_tok, rows}, {"row_pos", c.row_pos, rows}, {"row_win", c.row_win, rows},
        {"row_slot", c.row_slot, rows}, {"win_row0", c.win_row0, rows}, {"win_nrows", c.win_nrows, rows},
        {"win_slot", c.win_slot, rows}, {"rows_in", c.rows_in, rows}, {"src_rows", c.src_rows, rows},
        {"st_row_win", c.st_row_win, rows}, {"st_row_slot", c.st_row_slot, rows}, {"st_win_row0", c.st_win_row0, rows},
        {"st_win_nrows", c.st_win_nrows, rows}, {"st_win_slot", c.st_win_slot, rows},
        {"qk_map", c.qk_map, 2 * 2 * 4}, {"suppress", c.suppress, 1621 * 4}, {"d_seeks", c.d_seeks, 2 * 8},
        {"d_segs", c.d_segs, win}, {"S.hist", c.S.hist, 10 * 449 * 4}, {"S.anc", c.S.anc, 10 * 448 * 4},
        {"fp_anc", c.fp_anc, 2 * 448 * 4}, {"S.len", c.S.len, win}, {"S.sample_begin", c.S.sample_begin, win},
        {"S.step", c.S.step, win}, {"S.done", c.S.done, win}, {"S.fin_n", c.S.fin_n, win},
        {"S.sum_lp", c.S.sum_lp, 10 * 4}, {"S.fin_score", c.S.fin_score, 32 * 4}, {"S.fin_len", c.S.fin_len, 32 * 4},
        {"S.fin_tok", c.S.fin_tok, 32 * 449 * 4}, {"S.cand_val", c.S.cand_val, 90 * 4},
        {"S.cand_idx", c.S.cand_idx, 90 * 4}, {"S.lpart", c.S.lpart, 10 * 32 * 32 * 4}, {"S.lp_cnt", c.S.lp_cnt, 10 * 4},
        {"S.lpw_cnt", c.S.lpw_cnt, win}, {"S.seed", c.S.seed, 64},
        {"p1_slab", c.p1_slab, 2048 * 256 * 4}, {"p1_cnt", c.p1_cnt, 32 * 4},
        {"xs_rec", c.xs_rec, 2 * 2 * 24 * 1056 * 4}, {"xs_cnt", c.xs_cnt, 2 * 2 * 4}, {"x2_d", c.x2_d, 8 * 128 * 4},
        {"ekz_slab", c.ekz_slab, 24 * 65536}, {"ekz_cnt", c.ekz_cnt, 24 * 4 * 4}, {"bias_dev", c.bias_dev, 512 * 16}};
  });

  // the tensor tables: the count that wh_finalize asks for, by the formula it used to have
  // (89 for micro, 1259 for large-v3)
  CHECK(wh::n_loadable<Stand<T>>(2, 2) == 5 + 2 * 15 + 2 + 2 + 2 * 24 + 2, "%s: %zu loadable tensors for micro", dt,
        wh::n_loadable<Stand<T>>(2, 2));
  CHECK(wh::n_loadable<Stand<T>>(32, 32) == 5 + 32 * 15 + 2 + 2 + 32 * 24 + 2, "%s: %zu loadable tensors for large-v3",
        dt, wh::n_loadable<Stand<T>>(32, 32));
}

int main() {
  check_micro<uint16_t>();
  check_micro<float>();
  if (failures) return 1;
  puts("layout_host_check: ok");
  return 0;
}
