// The causal speech detector of live streams (wh_pool_vad_* / wh_stream_vad_*).  A translation
// unit of its own, as wh_vad.hip is.  The definition (absolute frame grid, sliding-window
// percentile, the run-length rules frame by frame) is in include/whisper_hip.h; whisper/vad.py
// (StreamVad) restates it in numpy.  Everything is integer arithmetic behind the quantisation.
#include "wh_svad.h"

namespace wh {

constexpr int SVAD_T = 256;            // threads of a workgroup: eight per frame of a pass
constexpr int SVAD_ROW = VAD_HOP + 8;  // as VAD_ROW of k_frame_energy

// One workgroup per detecting slot, two phases with one barrier between them.
//
// Energies.  The call's frame grid is the slot's absolute one seen from the incomplete frame the
// detector holds: virtual sample v = fill + j for new sample j, fill = state.samples % 160, so
// virtual frame k is samples [160 k, 160 k + 160) and only v in [fill, fill + n_new) exists.
// Virtual frame 0 lacks its first `fill` samples: their q^2 sum is state.partial.  A pass takes
// VAD_FB virtual frames as k_frame_energy takes a span of a file: 16-byte vectors from the
// aligned address below the span where a vector lies inside the new samples, guarded scalar
// loads at its edges, squares to LDS rows padded to SVAD_ROW, eight lanes summing a frame.
// energy[k] = the sum of virtual frame k (frame 0 with the partial added): whole frames and,
// last, the incomplete tail.
//
// Recurrence.  Wave 0 alone.  Lane l keeps the counters of bins 3 l, 3 l + 1, 3 l + 2 in
// registers (lanes 0..53 cover the 160 bins).  The wave takes min(64, window) frames at a time:
// lane i loads E of frame i, computes its bin, reads the ring entry that frame replaces and
// writes the new one (the ring positions of one such chunk are distinct); then the frames go one
// by one, everything about a frame broadcast from its lane: the counters move by one add and one
// remove, an inclusive prefix sum over the lanes' totals and a ballot find the first lane whose
// cumulative count reaches the rank, that lane picks among its three bins, and the state machine
// runs on wave-uniform values.  No barrier inside the loop.  The state block is written once.
__device__ __forceinline__ void svad_run(const SvadDesc& d, wh_svad_state* __restrict__ out, unsigned* sq) {
  SvadBlock* blk = d.block;
  const wh_svad_state s0 = blk->s;
  const wh_svad_opts o = blk->o;
  const int fill = (int)(s0.samples % VAD_HOP);
  const int64_t n_new = d.n_new;
  const int64_t end = fill + n_new;  // the virtual samples that exist are [fill, end)
  const int64_t K = svad_frames(fill, n_new);
  unsigned long long* energy = d.energy;

  for (int64_t c0 = 0; c0 < K; c0 += VAD_FB) {
    const int nf = K - c0 < VAD_FB ? (int)(K - c0) : VAD_FB;
    const int span = nf * VAD_HOP;
    const int64_t v0 = c0 * VAD_HOP;
    const int lo = fill > v0 ? (int)(fill - v0) : 0;           // the span's floats [lo, hi) exist
    const int hi = end - v0 < span ? (int)(end - v0) : span;
    const uintptr_t a = (uintptr_t)d.src + (uintptr_t)((intptr_t)4 * (intptr_t)(v0 - fill));  // the span's float 0
    const int head = (int)((a >> 2) & 3);
    const float* __restrict__ s = (const float*)a;
    const float4* __restrict__ v4 = (const float4*)(a - (uintptr_t)(4 * head));
    const int nvec = (head + span + 3) >> 2;
    for (int v = threadIdx.x; v < nvec; v += SVAD_T) {
      const int p0 = 4 * v - head;
      float x[4];
      if (p0 >= lo && p0 + 4 <= hi) {
        const float4 t = v4[v];
        x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = (p0 + j >= lo && p0 + j < hi) ? s[p0 + j] : 0.0f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int p = p0 + j;
        if (p >= 0 && p < span) sq[p + 8 * (p / VAD_HOP)] = vad_sq(x[j]);
      }
    }
    __syncthreads();
    const int fr = threadIdx.x >> 3, part = threadIdx.x & 7;
    unsigned long long sum = 0;
    if (fr < nf) {
      const unsigned* row = sq + fr * SVAD_ROW + part;
#pragma unroll
      for (int i = 0; i < VAD_HOP / 8; ++i) sum += row[8 * i];
    }
    sum += __shfl_xor(sum, 1);
    sum += __shfl_xor(sum, 2);
    sum += __shfl_xor(sum, 4);
    if (fr < nf && part == 0) energy[c0 + fr] = sum + (c0 + fr == 0 ? (unsigned long long)s0.partial : 0ull);
    __syncthreads();  // the rows are rewritten by the next pass
  }
  // the energies went through global memory: wave 0 reads them next
  __threadfence_block();
  __syncthreads();
  if (threadIdx.x >= 64) return;

  const int lane = threadIdx.x;
  const int64_t whole = end / VAD_HOP;
  const bool tail = end % VAD_HOP != 0;
  const int64_t n_close = whole + ((d.finish && tail) ? 1 : 0);  // at most K
  unsigned h0 = 3 * lane < VAD_BINS ? blk->hist[3 * lane] : 0u;
  unsigned h1 = 3 * lane + 1 < VAD_BINS ? blk->hist[3 * lane + 1] : 0u;
  unsigned h2 = 3 * lane + 2 < VAD_BINS ? blk->hist[3 * lane + 2] : 0u;
  uint8_t* ring = (uint8_t*)(blk + 1);
  const int W = o.window;
  int64_t frames = s0.frames, run_start = s0.run_start, run_end = s0.run_end;
  int64_t closed_start = s0.closed_start, closed_end = s0.closed_end, closed_total = s0.closed_total;
  unsigned long long threshold = s0.threshold;
  int state = s0.state;
  const int chunk = W < 64 ? W : 64;
  for (int64_t c = 0; c < n_close; c += chunk) {
    const int cl = n_close - c < chunk ? (int)(n_close - c) : chunk;
    unsigned long long my_e = 0;
    int my_bin = 0, my_old = 0;
    if (lane < cl) {
      my_e = energy[c + lane];
      my_bin = vad_bin(my_e);
      const int64_t f = frames + lane;
      uint8_t* r = ring + (int)(f % W);
      if (f >= W) my_old = *r;
      *r = (uint8_t)my_bin;
    }
    for (int i = 0; i < cl; ++i) {
      const unsigned long long e = __shfl(my_e, i);
      const int b = __shfl(my_bin, i), ob = __shfl(my_old, i);
      const int64_t f = frames;
      {
        const int l = b / 3, j = b - 3 * l;
        if (lane == l) { h0 += j == 0; h1 += j == 1; h2 += j == 2; }
      }
      if (f >= W) {
        const int l = ob / 3, j = ob - 3 * l;
        if (lane == l) { h0 -= j == 0; h1 -= j == 1; h2 -= j == 2; }
      }
      const int64_t n = f + 1 < W ? f + 1 : W;
      int64_t rank64 = (n * o.percentile + 99) / 100;
      const unsigned rank = rank64 < 1 ? 1u : (unsigned)rank64;
      const unsigned mine = h0 + h1 + h2;
      unsigned inc = mine;
#pragma unroll
      for (int dl = 1; dl < 64; dl <<= 1) {
        const unsigned t = __shfl_up(inc, dl);
        if (lane >= dl) inc += t;
      }
      const unsigned long long reached = __ballot(inc >= rank);
      const int first = reached ? __ffsll((long long)reached) - 1 : 53;  // the counts sum to n >= rank
      const unsigned exc = inc - mine;
      int bin = 3 * lane + (exc + h0 >= rank ? 0 : (exc + h0 + h1 >= rank ? 1 : 2));
      bin = __shfl(bin, first);
      bin = bin < VAD_BINS - 1 ? bin : VAD_BINS - 1;
      unsigned long long T = (vad_edge(bin) * o.ratio_q8) >> 8;
      T = T < o.t_lo ? o.t_lo : T;
      T = T > o.t_hi ? o.t_hi : T;
      if (e > T) {
        if (state == 0) { state = 1; run_start = f; }
        run_end = f + 1;
        if (state == 1 && run_end - run_start >= o.min_speech) state = 2;
      } else if (state != 0 && f + 1 - run_end >= o.min_silence) {
        if (state == 2) { closed_start = run_start; closed_end = run_end; ++closed_total; }
        state = 0;
      }
      frames = f + 1;
      threshold = T;
    }
    __threadfence_block();  // the ring entries of this chunk, before the next chunk reads the ring
  }
  if (3 * lane < VAD_BINS) blk->hist[3 * lane] = h0;
  if (3 * lane + 1 < VAD_BINS) blk->hist[3 * lane + 1] = h1;
  if (3 * lane + 2 < VAD_BINS) blk->hist[3 * lane + 2] = h2;
  if (lane == 0) {
    wh_svad_state r;
    r.frames = frames; r.samples = s0.samples + n_new;
    r.run_start = run_start; r.run_end = run_end;
    r.closed_start = closed_start; r.closed_end = closed_end; r.closed_total = closed_total;
    r.threshold = threshold;
    r.partial = (tail && !d.finish) ? energy[whole] : 0ull;
    r.state = state; r.reserved = 0;
    blk->s = r;
    out[d.out_index] = r;
  }
}

__global__ __launch_bounds__(SVAD_T) void k_stream_vad_pool(const SvadDesc* __restrict__ descs,
                                                            wh_svad_state* __restrict__ out) {
  __shared__ unsigned sq[VAD_FB * SVAD_ROW];
  svad_run(descs[blockIdx.x], out, sq);
}
__global__ __launch_bounds__(SVAD_T) void k_stream_vad_one(SvadDesc desc, wh_svad_state* __restrict__ out) {
  __shared__ unsigned sq[VAD_FB * SVAD_ROW];
  svad_run(desc, out, sq);
}

void launch_stream_vad_pool(const SvadDesc* descs, int n, wh_svad_state* out, hipStream_t st) {
  if (n < 1) return;
  k_stream_vad_pool<<<n, SVAD_T, 0, st>>>(descs, out), wh_launched("k_stream_vad_pool");
}
void launch_stream_vad_one(const SvadDesc& desc, wh_svad_state* out, hipStream_t st) {
  k_stream_vad_one<<<1, SVAD_T, 0, st>>>(desc, out), wh_launched("k_stream_vad_one");
}

}  // namespace wh
