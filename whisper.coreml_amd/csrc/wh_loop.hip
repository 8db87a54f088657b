// DecodeLoop (csrc/wh_loop.h): host code only, no kernel is defined or instantiated here.
#include "wh_loop.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

using namespace wh;

static size_t al256(size_t b) { return (b + 255) & ~size_t(255); }

int DecodeLoop::set_opts(const wh_decode_opts* o, int n_win) {
  // every refusal comes before the first write: a refused call leaves O, S and maxc alone
  if (o->group < 1 || o->group > Gcap) return fail(-11, "group exceeds context max_group");
  // max_candidates = round(beam_size * patience) (decoding.py:339): Python rounds half
  // to even; the host passes its own value, else nearbyint (default mode: half to even)
  const int mc = !o->beam ? 0
                 : o->max_candidates > 0 ? o->max_candidates
                                         : (int)std::nearbyint((double)o->group * (o->patience > 0 ? o->patience : 1.0));
  if (o->beam && (mc < 1 || mc > 16)) return fail(-11, "max_candidates out of range (1..16)");
  if (o->no_repeat_ngram < 0 || o->no_repeat_ngram > 16)
    return fail(-11, "no_repeat_ngram " + std::to_string(o->no_repeat_ngram) + " out of range (0..16)");
  if (!(o->repetition_penalty >= 0.f) || std::isinf(o->repetition_penalty))
    return fail(-11, "repetition_penalty must be finite and not negative (0 or 1: off)");
  const float pen = o->repetition_penalty == 0.f ? 1.f : o->repetition_penalty;
  const bool rep_on = o->no_repeat_ngram > 0 || pen != 1.f;
  if (rep_on || !bias_tab.empty()) {
    // the history filters exist in the sliced selection only
    DecOpts q = DecOpts();
    q.V = V; q.ts_begin = o->timestamp_begin;
    if (!logit_slices(S, q, n_win))
      return fail(-11, std::string(!rep_on ? "phrase_bias" : bias_tab.empty() ? "no_repeat_ngram / repetition_penalty"
                                                                : "no_repeat_ngram / repetition_penalty / phrase_bias") +
                           " need the sliced selection (k_logit_part): not with this vocabulary or "
                           "WHISPER_HIP_LOGIT_SPLIT=0");
  }
  for (size_t e = 0; e < bias_tab.size(); ++e)
    if (bias_tab[e].id >= o->eot) {
      const int j = (int)std::count_if(bias_tab.begin(), bias_tab.begin() + e + 1, [](const BiasRec& r) { return r.k == 0; }) - 1;
      return fail(-11, "phrase_bias: phrase " + std::to_string(j) + " names id " + std::to_string(bias_tab[e].id) +
                           ", not a text id (eot " + std::to_string(o->eot) + ")");
    }
  O = DecOpts();
  O.no_repeat_ngram = o->no_repeat_ngram; O.repetition_penalty = pen;
  // the table as it is now, for this decode; the pointer and the count are all DecOpts sees
  O.n_bias = (int)bias_tab.size();
  O.bias = O.n_bias ? bias_dev : nullptr;
  if (O.n_bias)
    HIPCHK(hipMemcpyAsync(bias_dev, bias_tab.data(), bias_tab.size() * sizeof(BiasRec), hipMemcpyHostToDevice, st));
  O.V = V; O.eot = o->eot; O.ts_begin = o->timestamp_begin; O.no_ts = o->no_timestamps;
  O.n_blank = std::min(o->n_blank, 3);
  for (int i = 0; i < O.n_blank; ++i) O.blank[i] = o->blank[i];
  O.blank[O.n_blank] = o->eot;  // SuppressBlank masks encode(" ") + [eot]
  O.n_blank += 1;
  O.suppress_blank = o->suppress_blank; O.timestamps = o->timestamps; O.max_initial = o->max_initial;
  O.beam = o->beam; O.sample_len = o->sample_len; O.n_ctx = CTX; O.temperature = o->temperature;
  h_seed = o->seed;
  std::vector<unsigned> mask((V + 31) / 32, 0u);
  for (int i = 0; i < o->n_suppress; ++i) {
    const int t = o->suppress[i];
    if (t >= 0 && t < V) mask[t >> 5] |= 1u << (t & 31);
  }
  HIPCHK(hipMemcpyAsync(suppress, mask.data(), mask.size() * 4, hipMemcpyHostToDevice, st));
  O.suppress = o->n_suppress > 0 ? suppress : nullptr;
  maxc = mc;
  S.G = o->group;
  S.maxc = 16;
  return 0;
}

int DecodeLoop::begin_check(int n_win, int G, const int* init, const int* n_init, int max_init, const int* sot_index,
                            const int* slots) {
  if (!finalized) return fail(-9, "weights not finalized");
  // no usable batch until this one is fully set up: a failure below leaves neither the
  // device loop nor the per-step ABI (wh_step / wh_reorder_kv) a half-written batch
  cur_nwin = 0;
  step_api = false;
  if (n_win < 1 || n_win > Wcap) return fail(-11, "n_win out of range");
  if (G < 1 || G > Gcap) return fail(-11, "group exceeds context max_group");
  win_slots.resize(n_win);
  for (int w = 0; w < n_win; ++w) {
    win_slots[w] = slots ? slots[w] : w;
    if (win_slots[w] < 0 || win_slots[w] >= Wcap) return fail(-11, "window slot out of range");
  }
  for (int w = 0; w < n_win; ++w) {
    if (n_init[w] < 1 || n_init[w] > CTX - 1) return fail(-11, "initial token count out of range");
    if (sot_index[w] < 0 || sot_index[w] >= n_init[w]) return fail(-11, "bad sot_index");
    for (int p = 0; p < n_init[w]; ++p) {
      const int t = init[(size_t)w * max_init + p];
      if (t < 0 || t >= V) return fail(-11, "initial token out of vocabulary");
    }
  }
  return 0;
}

int DecodeLoop::step_check(const int* tok, const int* offsets) {
  if (!step_api || cur_nwin < 1) return fail(-13, "no per-step batch (call wh_prefill first)");
  const int R = cur_nwin * cur_G;
  for (int r = 0; r < R; ++r)
    if (tok[r] < 0 || tok[r] >= V) return fail(-13, "step token out of vocabulary");
  for (int w = 0; w < cur_nwin; ++w) {
    if (h_len[w] >= CTX) return fail(-13, "text context full (448 positions)");
    if (offsets && offsets[w] != h_len[w])
      return fail(-13, "text_offset " + std::to_string(offsets[w]) + " of window " + std::to_string(w) +
                           " != cached length " + std::to_string(h_len[w]));
  }
  return 0;
}

int DecodeLoop::reorder_kv(const int* src) {
  if (!step_api || cur_nwin < 1) return fail(-13, "no per-step batch (call wh_prefill first)");
  const int R = cur_nwin * cur_G;
  for (int r = 0; r < R; ++r)
    if (src[r] / cur_G != r / cur_G || src[r] < 0)
      return fail(-13, "source row " + std::to_string(src[r]) + " of row " + std::to_string(r) +
                           " is not a row of the same window");
  HIPCHK(hipMemcpyAsync(src_rows, src, R * 4, hipMemcpyHostToDevice, st));
  launch_reorder_rows(S, src_rows, cur_nwin, st);
  HIPCHK(hipStreamSynchronize(st));
  TRY(launch_status(__func__));
  return 0;
}

int DecodeLoop::ensure_graph() {
  std::vector<char> key(sizeof(DecOpts) + sizeof(DecState) + 8);
  memcpy(key.data(), &O, sizeof(DecOpts));
  memcpy(key.data() + sizeof(DecOpts), &S, sizeof(DecState));
  memcpy(key.data() + sizeof(DecOpts) + sizeof(DecState), &cur_nwin, 4);
  memcpy(key.data() + sizeof(DecOpts) + sizeof(DecState) + 4, &cur_G, 4);
  if (gexec && key == graph_key) return 0;
  if (gexec) { hipGraphExecDestroy(gexec); gexec = nullptr; }
  if (graph) { hipGraphDestroy(graph); graph = nullptr; }
  HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  const int rc = step_body();
  hipGraph_t g = nullptr;
  const hipError_t e = hipStreamEndCapture(st, &g);
  if (rc) { if (g) hipGraphDestroy(g); return rc; }
  if (e != hipSuccess) return fail(-12, std::string("graph capture: ") + hipGetErrorString(e));
  graph = g;
  HIPCHK(hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0));
  graph_key = key;
  return 0;
}

int DecodeLoop::launch_step() {
  if (eager()) return step_body();
  HIPCHK(hipGraphLaunch(gexec, st));
  return 0;
}

int DecodeLoop::decode_steps(int max_steps, int* n_done) {
  if (cur_nwin < 1) return fail(-13, "no decode in progress");
  if (step_api) return fail(-13, "the batch was begun with wh_prefill (per-step mode): use wh_step");
  if (!eager()) TRY(ensure_graph());
  TRY(tm.mark(0, st));
  restore_rows();
  int steps = 0, done = 0;
  static const int chunk = [] {  // WHISPER_HIP_POLL_CHUNK: steps per done-flag poll (A/B)
    const char* e = tune_env("WHISPER_HIP_POLL_CHUNK");
    const int v = e ? atoi(e) : 8;
    return v < 1 ? 1 : v;
  }();
  // chunks of `chunk` steps, each followed by an async copy of the done flags; the
  // next chunk is queued before the host waits for the previous chunk's flags, so
  // the GPU never idles on the poll (at most one chunk of no-op steps after the last
  // window finishes: finished windows' rows are clamped and skipped by the selection)
  auto queue_chunk = [&](int b) -> int {
    const int k = std::min(chunk, max_steps - steps);
    for (int i = 0; i < k; ++i) TRY(launch_step());
    steps += k;
    HIPCHK(hipMemcpyAsync(h_done + b * Wcap, S.done, cur_nwin * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(poll_ev[b], st));
    return k;
  };
  auto tc = std::chrono::steady_clock::now();
  int b = 0, kq[2] = {0, 0};
  kq[0] = queue_chunk(0);
  if (kq[0] < 0) return kq[0];
  while (true) {
    const int nb = b ^ 1;
    kq[nb] = steps < max_steps ? queue_chunk(nb) : 0;
    if (kq[nb] < 0) return kq[nb];
    HIPCHK(hipEventSynchronize(poll_ev[b]));
    // per-token wall time (graph launches + done poll, pipelined), for the p50
    const auto now = std::chrono::steady_clock::now();
    token_ms.push_back((float)(std::chrono::duration<double, std::milli>(now - tc).count() / kq[b]));
    tc = now;
    done = 0;
    for (int w = 0; w < cur_nwin; ++w) done += h_done[b * Wcap + w] != 0;
    if (done == cur_nwin || kq[nb] == 0) break;
    b = nb;
  }
  TRY(tm.finish(st, stats[WH_STAT_STEPS_MS]));
  stats[WH_STAT_STEPS] += steps;
  *n_done = done;
  return 0;
}

int DecodeLoop::decode_read(int slot, int* tokens, float* slp, int* len, int* fin_n, int* fin_tok, int* fin_len,
                            float* fin_score, float* nspo) {
  if (slot < 0 || slot >= cur_nwin) return fail(-14, "slot");
  const int G = cur_G;
  HIPCHK(hipStreamSynchronize(st));
  if (tokens) HIPCHK(hipMemcpy(tokens, S.hist + (size_t)slot * G * HCTX, (size_t)G * HCTX * 4, hipMemcpyDeviceToHost));
  if (slp) HIPCHK(hipMemcpy(slp, S.sum_lp + slot * G, G * 4, hipMemcpyDeviceToHost));
  if (len) HIPCHK(hipMemcpy(len, S.len + slot, 4, hipMemcpyDeviceToHost));
  if (fin_n) HIPCHK(hipMemcpy(fin_n, S.fin_n + slot, 4, hipMemcpyDeviceToHost));
  const int mc = S.maxc;
  if (fin_tok) HIPCHK(hipMemcpy(fin_tok, S.fin_tok + (size_t)slot * mc * HCTX, (size_t)mc * HCTX * 4, hipMemcpyDeviceToHost));
  if (fin_len) HIPCHK(hipMemcpy(fin_len, S.fin_len + slot * mc, mc * 4, hipMemcpyDeviceToHost));
  if (fin_score) HIPCHK(hipMemcpy(fin_score, S.fin_score + slot * mc, mc * 4, hipMemcpyDeviceToHost));
  if (nspo) HIPCHK(hipMemcpy(nspo, nsp + slot, 4, hipMemcpyDeviceToHost));
  return 0;
}

int DecodeLoop::check_slot_idle(int slot) {
  if (cur_nwin < 1 || step_api) return 0;
  for (int w = 0; w < cur_nwin; ++w)
    if (win_slots[w] == slot) {
      int d = 0;
      HIPCHK(hipMemcpyAsync(&d, S.done + w, 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (!d)
        return fail(-15, "slot " + std::to_string(slot) + " is still decoding (window " + std::to_string(w) +
                             " of the current batch): a first pass would overwrite its self-KV rows");
    }
  return 0;
}

int DecodeLoop::ensure_scratch(size_t bytes) {
  if (bytes <= scratch.cap) return 0;
  HIPCHK(hipStreamSynchronize(st));
  return scratch.reserve(bytes);
}

int DecodeLoop::dtw(const float* x, int N, int M, int* path, int* plen, const DtwOpen* open) {
  const std::string who = open ? "dtw_open" : "dtw";  // wh_dtw_open checks its shape before the context is entered
  if (!open && (N < 1 || M < 1 || N > 1023 || (int64_t)N * M > (int64_t)1 << 26))
    return fail(-15, "dtw: shape out of range");
  const size_t b_x = al256((size_t)N * M * 4), b_tr = al256(dtw_trace_bytes(N, M)), b_path = al256((size_t)2 * (N + M) * 4),
               b_sc = open ? al256((size_t)N * 4) : 0;
  TRY(ensure_scratch(b_x + b_tr + b_path + b_sc + 256 + al256(sizeof(DtwJob))));
  char* p = scratch.p;
  float* d_x = (float*)p; p += b_x;
  unsigned* d_tr = (unsigned*)p; p += b_tr;
  int* d_path = (int*)p; p += b_path;
  float* d_sc = (float*)p; p += b_sc;
  int* d_plen = (int*)p; p += 256;  // [0] path length, [1] end row (open)
  DtwJob* d_job = (DtwJob*)p;
  DtwJob job{d_x, d_tr, d_path, d_plen, N, M, 0};
  if (open) {
    job.min_rows = open->min_rows ? open->min_rows : N;
    job.row_penalty = open->row_penalty;
    job.end_row = d_plen + 1;
    job.scores = open->scores ? d_sc : nullptr;
  }
  size_t lds = 0;
  if (dtw_prepare(&job, 1, &lds)) return fail(-15, who + ": shape");
  HIPCHK(hipMemcpyAsync(d_x, x, (size_t)N * M * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_job, &job, sizeof(job), hipMemcpyHostToDevice, st));
  if (launch_dtw_jobs(d_job, 1, N, job.in_lds, lds, 1.f, open != nullptr, st)) return fail(-15, who + " launch");
  int pe[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(pe, d_plen, open ? 8 : 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(path, d_path, (size_t)2 * (N + M) * 4, hipMemcpyDeviceToHost, st));
  if (open && open->scores) HIPCHK(hipMemcpyAsync(open->scores, d_sc, (size_t)N * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  TRY(launch_status(who.c_str()));
  *plen = pe[0];
  if (open) *open->end_row = pe[1];
  return 0;
}

int DecodeLoop::align_windows(int n_win, const int* slots, const int* tokens, const int* n_tokens, int n_sot,
                              const int* num_frames, const int* ah, int na, int medfilt, const int* min_rows,
                              float row_penalty, float* probs, int* paths, int* plens, int* end_rows) {
  if (!finalized) return fail(-9, "weights not finalized");
  if (n_win < 1) return fail(-15, "align: no windows");
  if (na < 1 || na > Ld * nh) return fail(-15, "align: alignment head count");
  if (medfilt < 1 || medfilt > 15 || medfilt % 2 == 0) return fail(-15, "align: medfilt_width must be odd <= 15");
  std::vector<int64_t> tok_off(n_win + 1, 0), prob_off(n_win + 1, 0), path_off(n_win + 1, 0), mat_off(n_win + 1, 0),
      tr_off(n_win + 1, 0);
  int rows_max = 0;
  for (int w = 0; w < n_win; ++w) {
    const int n = n_tokens[w], Tt = n - n_sot - 2, F = num_frames[w] / 2;
    if (n_sot < 1 || Tt < 1) return fail(-15, "align: need sot_sequence + no_timestamps + >= 1 text token + eot");
    if (n > CTX) return fail(-15, "align: more than 448 tokens");
    if (F < 1 || F > 1500) return fail(-15, "align: num_frames out of range");
    if (slots[w] < 0 || slots[w] >= Wcap) return fail(-15, "align: bad slot");
    TRY(check_slot_idle(slots[w]));
    const int N = Tt + 1;
    tok_off[w + 1] = tok_off[w] + n;
    prob_off[w + 1] = prob_off[w] + Tt;
    path_off[w + 1] = path_off[w] + 2 * (N + F);
    mat_off[w + 1] = mat_off[w] + ((int64_t)N * F + 63) / 64 * 64;
    tr_off[w + 1] = tr_off[w] + (dtw_trace_bytes(N, F) + 255) / 256 * 256;
    rows_max = std::max(rows_max, n);
  }
  // pass grouping: consecutive windows while the rows fit PRE and the cross-QK budget
  const int64_t qk_row = (int64_t)na * 1500 * 4;
  const int cap = (int)std::max<int64_t>(rows_max, std::min<int64_t>(PRE, ((int64_t)1 << 30) / qk_row));
  const size_t b_qk = al256((size_t)qk_row * cap), b_lg = al256((size_t)128 * V * 4), b_mat = al256(mat_off[n_win] * 4),
               b_tr = al256(tr_off[n_win]), b_path = al256(path_off[n_win] * 4), b_pr = al256(prob_off[n_win] * 4 + 16),
               b_pl = al256((size_t)n_win * 4), b_jobs = al256((size_t)n_win * sizeof(DtwJob));
  TRY(ensure_scratch(b_qk + b_lg + b_mat + b_tr + b_path + 2 * b_pr + 2 * b_pl + b_jobs));
  char* p = scratch.p;
  float* d_qk = (float*)p; p += b_qk;
  float* d_lg = (float*)p; p += b_lg;
  float* d_mat = (float*)p; p += b_mat;
  char* d_tr = p; p += b_tr;
  int* d_path = (int*)p; p += b_path;
  float* d_probs = (float*)p; p += b_pr;
  int* d_ptok = (int*)p; p += b_pr;
  int* d_plen = (int*)p; p += b_pl;
  int* d_end = (int*)p; p += b_pl;
  DtwJob* d_jobs = (DtwJob*)p;

  // token of every probability row (timing.py:191: text_tokens[k])
  std::vector<int> ptok(prob_off[n_win]);
  for (int w = 0; w < n_win; ++w)
    for (int k = 0; k < prob_off[w + 1] - prob_off[w]; ++k) ptok[prob_off[w] + k] = tokens[tok_off[w] + n_sot + 1 + k];
  HIPCHK(hipMemcpyAsync(d_ptok, ptok.data(), ptok.size() * 4, hipMemcpyHostToDevice, st));
  std::vector<int> map((size_t)Ld * nh, -1);
  for (int i = 0; i < na; ++i)
    if (ah[i] >= 0 && ah[i] < Ld * nh) map[ah[i]] = i;
  HIPCHK(hipMemcpyAsync(qk_map, map.data(), map.size() * 4, hipMemcpyHostToDevice, st));
  std::vector<DtwJob> jobs(n_win);
  const int eot = tokens[tok_off[1] - 1];
  for (int w0 = 0; w0 < n_win;) {
    int nw = 0, R = 0;
    while (w0 + nw < n_win && (nw == 0 || R + n_tokens[w0 + nw] <= cap)) R += n_tokens[w0 + nw++];
    // rows of this pass: window slot, beam slot 0, position; sel: the rows that predict text
    RowPlan rows;
    std::vector<int> sel;
    for (int i = 0; i < nw; ++i) {
      const int w = w0 + i, n = n_tokens[w];
      rows.add(slots[w], slots[w], tokens + tok_off[w], n);
      for (int k = 0; k < n - n_sot - 2; ++k) sel.push_back(rows.win_row0[i] + n_sot + k);
      if (tokens[tok_off[w] + n - 1] != eot) return fail(-15, "align: windows must end with the same eot");
    }
    for (int q = 0; q < R; ++q)
      if (rows.row_tok[q] < 0 || rows.row_tok[q] >= V) return fail(-15, "align: token out of vocabulary");
    const int64_t pb = prob_off[w0];
    TRY(align_rows(rows, sel, d_qk, d_lg, eot, d_ptok + pb, d_probs + pb));
    for (int i = 0; i < nw; ++i) {
      const int w = w0 + i, N = n_tokens[w] - n_sot - 1, F = num_frames[w] / 2;
      float* mat = d_mat + mat_off[w];
      launch_align_matrix(d_qk + (int64_t)rows.win_row0[i] * 1500, (int64_t)R * 1500, n_tokens[w], 1500, F, na, n_sot, N,
                          medfilt, mat, st);
      jobs[w] = DtwJob{mat, (unsigned*)(d_tr + tr_off[w]), d_path + path_off[w], d_plen + w, N, F, 0};
      if (min_rows) {
        jobs[w].min_rows = min_rows[w] ? min_rows[w] : N;
        jobs[w].row_penalty = row_penalty;
        jobs[w].end_row = d_end + w;
      }
    }
    size_t lds = 0;
    if (dtw_prepare(jobs.data() + w0, nw, &lds)) return fail(-15, "align: DTW shape");
    HIPCHK(hipMemcpyAsync(d_jobs + w0, jobs.data() + w0, nw * sizeof(DtwJob), hipMemcpyHostToDevice, st));
    int max_n = 0;
    for (int i = 0; i < nw; ++i) max_n = std::max(max_n, jobs[w0 + i].N);
    if (launch_dtw_jobs(d_jobs + w0, nw, max_n, jobs[w0].in_lds, lds, -1.f, min_rows != nullptr, st))
      return fail(-15, "align: DTW launch");
    HIPCHK(hipStreamSynchronize(st));  // the row plan and sel of this pass go out of scope
    w0 += nw;
  }
  HIPCHK(hipMemcpyAsync(probs, d_probs, prob_off[n_win] * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(plens, d_plen, n_win * 4, hipMemcpyDeviceToHost, st));
  if (min_rows) HIPCHK(hipMemcpyAsync(end_rows, d_end, n_win * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(paths, d_path, path_off[n_win] * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  TRY(launch_status(__func__));
  return 0;
}

int DecodeLoop::vocab_score_check(const float* x, int n_rows, const int* targets, const float* logprob, const int* top_id,
                                  const float* top_logprob) {
  const char* null = !x ? "x" : !targets ? "targets" : !logprob ? "logprob" : !top_id ? "top_id" : !top_logprob ? "top_logprob" : nullptr;
  if (null) return fail(-1, std::string("wh_vocab_score: null argument (") + null + ")");
  if (n_rows < 1 || n_rows > 4096) return fail(-15, "wh_vocab_score: n_rows = " + std::to_string(n_rows) + " outside 1..4096");
  for (int r = 0; r < n_rows; ++r)
    if (targets[r] < 0 || targets[r] >= V)
      return fail(-15, "wh_vocab_score: targets[" + std::to_string(r) + "] = " + std::to_string(targets[r]) +
                           " outside [0, " + std::to_string(V) + ")");
  if (!finalized) return fail(-9, "wh_vocab_score: weights not finalized");
  return 0;
}

int DecodeLoop::vocab_score(const float* x, int n_rows, const int* targets, float* logprob, int* top_id,
                            float* top_logprob) {
  const int ns = nh * 64;
  const size_t b_x = al256((size_t)SCORE_PASS * ns * 4), b_rec = al256(score_rec_bytes(SCORE_PASS)),
               b_o = al256((size_t)SCORE_PASS * 4);
  TRY(ensure_scratch(2 * b_x + b_rec + 4 * b_o));
  char* p = scratch.p;
  float* d_xf = (float*)p; p += b_x;
  void* d_xt = p; p += b_x;
  void* d_rec = p; p += b_rec;
  int* d_tgt = (int*)p; p += b_o;
  float* d_lp = (float*)p; p += b_o;
  int* d_top = (int*)p; p += b_o;
  float* d_tlp = (float*)p;
  for (int r0 = 0; r0 < n_rows; r0 += SCORE_PASS) {
    const int n = std::min(SCORE_PASS, n_rows - r0);
    HIPCHK(hipMemcpyAsync(d_xf, x + (size_t)r0 * ns, (size_t)n * ns * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_tgt, targets + r0, n * 4, hipMemcpyHostToDevice, st));
    TRY(score_host_rows(d_xf, d_xt, n, ScoreOut{d_tgt, d_rec, d_lp, d_top, d_tlp}));
    HIPCHK(hipMemcpyAsync(logprob + r0, d_lp, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(top_id + r0, d_top, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(top_logprob + r0, d_tlp, n * 4, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  TRY(launch_status(__func__));
  return 0;
}

int DecodeLoop::score_check(int n_seq, const int* slots, const int* tokens, const int* n_tokens, const int* n_ctx,
                            const float* logprob, const int* top_id, const float* top_logprob) {
  const char* null = !slots ? "slots" : !tokens ? "tokens" : !n_tokens ? "n_tokens" : !n_ctx ? "n_ctx" : !logprob ? "logprob"
                     : !top_id ? "top_id" : !top_logprob ? "top_logprob" : nullptr;
  if (null) return fail(-1, std::string("wh_score_batch: null argument (") + null + ")");
  if (n_seq < 1) return fail(-15, "wh_score_batch: n_seq = " + std::to_string(n_seq) + " below 1");
  auto at = [](const char* field, int i, int v) { return std::string("wh_score_batch: ") + field + "[" + std::to_string(i) + "] = " + std::to_string(v); };
  int64_t off = 0;
  for (int s = 0; s < n_seq; ++s) {
    if (slots[s] < 0 || slots[s] >= Wcap) return fail(-15, at("slots", s, slots[s]) + " outside 0.." + std::to_string(Wcap - 1));
    if (n_tokens[s] < 2 || n_tokens[s] > CTX) return fail(-15, at("n_tokens", s, n_tokens[s]) + " outside 2.." + std::to_string(CTX));
    if (n_ctx[s] < 1 || n_ctx[s] > n_tokens[s] - 1)
      return fail(-15, at("n_ctx", s, n_ctx[s]) + " outside 1.." + std::to_string(n_tokens[s] - 1));
    for (int i = 0; i < n_tokens[s]; ++i)
      if (tokens[off + i] < 0 || tokens[off + i] >= V)
        return fail(-15, at("tokens", (int)(off + i), tokens[off + i]) + " outside [0, " + std::to_string(V) + ") (id " +
                             std::to_string(i) + " of sequence " + std::to_string(s) + ")");
    off += n_tokens[s];
  }
  if (!finalized) return fail(-9, "wh_score_batch: weights not finalized");
  return 0;
}

int DecodeLoop::score_windows(int n_seq, const int* slots, const int* tokens, const int* n_tokens, const int* n_ctx,
                              float* logprob, int* top_id, float* top_logprob) {
  // the self-KV windows a sequence may borrow: every one the live batch is not decoding in
  std::vector<int> idle;
  for (int w = 0; w < Wcap; ++w) {
    const int rc = check_slot_idle(w);
    if (rc == 0) idle.push_back(w);
    else if (rc != -15) return rc;
  }
  if (idle.empty()) return fail(-15, "wh_score_batch: every self-KV window is still decoding");
  std::vector<int64_t> tok_off(n_seq + 1, 0), out_off(n_seq + 1, 0);
  for (int s = 0; s < n_seq; ++s) {
    tok_off[s + 1] = tok_off[s] + n_tokens[s];
    out_off[s + 1] = out_off[s] + n_tokens[s] - n_ctx[s];
  }
  const size_t b_rows = al256((size_t)PRE * 4), b_rec = al256(score_rec_bytes(PRE)), b_out = al256(out_off[n_seq] * 4);
  TRY(ensure_scratch(2 * b_rows + b_rec + 3 * b_out));
  char* p = scratch.p;
  int* d_sel = (int*)p; p += b_rows;
  int* d_tgt = (int*)p; p += b_rows;
  void* d_rec = p; p += b_rec;
  float* d_lp = (float*)p; p += b_out;
  int* d_top = (int*)p; p += b_out;
  float* d_tlp = (float*)p;
  for (int s0 = 0; s0 < n_seq;) {
    // rows of this pass: the borrowed window, beam slot 0, position; sel: the rows that are scored
    RowPlan rows;
    std::vector<int> sel, tgt;
    int nw = 0;
    while (s0 + nw < n_seq && nw < (int)idle.size() && rows.R + n_tokens[s0 + nw] - 1 <= PRE) {
      const int s = s0 + nw, n = n_tokens[s];
      const int* t = tokens + tok_off[s];
      rows.add(idle[nw], slots[s], t, n - 1);
      for (int i = n_ctx[s]; i < n; ++i) {
        sel.push_back(rows.win_row0[nw] + i - 1);
        tgt.push_back(t[i]);
      }
      ++nw;
    }
    HIPCHK(hipMemcpyAsync(d_sel, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_tgt, tgt.data(), tgt.size() * 4, hipMemcpyHostToDevice, st));
    const int64_t ob = out_off[s0];
    TRY(score_rows(rows, d_sel, (int)sel.size(), ScoreOut{d_tgt, d_rec, d_lp + ob, d_top + ob, d_tlp + ob}));
    HIPCHK(hipStreamSynchronize(st));  // the row plan, sel and tgt of this pass go out of scope
    s0 += nw;
  }
  HIPCHK(hipMemcpyAsync(logprob, d_lp, out_off[n_seq] * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(top_id, d_top, out_off[n_seq] * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(top_logprob, d_tlp, out_off[n_seq] * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  TRY(launch_status(__func__));
  return 0;
}
