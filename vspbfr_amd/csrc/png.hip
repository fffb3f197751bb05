// Device-side PNG encoder for gfx950: row filters + deflate of a (B, H, W, C) uint8 batch (format and limits: include/vspbfr_hip.h;
// the host restatement every byte is held to: tests/png_ref.py).
//
// One launch, one workgroup of 512 threads (8 waves) per (image, segment of VSP_PNG_SEG_ROWS rows):
//   load      the segment's rows and the row above it with aligned dword loads over the byte stream into LDS (an NHWC row of C * W bytes
//             is not dword aligned in general: the LDS copy keeps the misalignment of the global range, so a global dword is an LDS
//             dword; only dwords that straddle the ends of the tensor are assembled from bytes)
//   filter    one wave per row: the five |int8| residual sums in one sweep, a wave reduction, the chosen residuals into LDS
//   tokens    a thread owns a contiguous chunk of the segment's bytes; the start and the end of the stretch of repeated bytes a position
//             lies in come from a forward max-scan and a backward min-scan over the chunks
//   codes     histogram with LDS atomics; code lengths: a parallel rank sort, then one thread does the two-queue merge, the depth
//             counts and the limit repair; canonical codes in parallel
//   bits      per-chunk bit counts, a prefix sum, then every token is or-ed into the LDS bit buffer (two threads may share a dword there)
//   store     the finished buffer goes to the segment's slot as plain dword stores; byte count and Adler parts beside it
// The bit buffer reuses the LDS of the raw rows.  Static LDS only (below 64 KB); no scratch: every dynamically indexed array is in LDS.
// Everything from `tokens` on is compress_segment(), which the ragged encoder for whole photos (further down: three kernels, segments of
// VSP_PNG_RAGGED_SEG_BYTES bytes instead of rows) calls on filtered bytes it rebuilds from global memory.
#include "vsp_common.h"

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kRows = VSP_PNG_SEG_ROWS;
constexpr int kMaxRow = VSP_PNG_MAX_ROW_BYTES;
constexpr int kMaxSeg = kRows * (kMaxRow + 1);               // filtered bytes of a segment
constexpr int kRawDwords = ((kRows + 1) * kMaxRow + 3) / 4 + 1;   // the rows, the row above, 3 bytes of misalignment
constexpr int kLit = 286, kClSyms = 19, kMaxClTok = 320;
constexpr uint32_t kAdler = 65521u;
static_assert(kRawDwords * 4 >= kMaxSeg + 16, "the bit buffer (a stored segment at most) lives in the raw rows' LDS");
static_assert(kMaxSeg < 65536, "one stored block per segment");

__constant__ uint8_t kClOrder[kClSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__host__ __device__ inline int seg_bound(int rows, int rb) { return (rows * (rb + 1) + 10 + 3) / 4 * 4; }

struct Huff {                 // work arrays of build_code (all in LDS)
  int nodew[kLit];            // weights of the internal nodes, in creation order
  uint16_t sorted[kLit];      // used symbols by (count, symbol)
  uint16_t leafpar[kLit], nodepar[kLit], depth[kLit];
  int count[16], next[16];
};

// inclusive scan over the workgroup in thread order `idx` (a permutation of 0..kThreads-1); returns the buffer holding the result
template <class Op>
__device__ __forceinline__ const int* block_scan(int v, int idx, int (*sh)[kThreads], Op op) {
  int cur = 0;
  sh[0][idx] = v;
  __syncthreads();
  for (int d = 1; d < kThreads; d <<= 1) {
    int x = sh[cur][idx];
    if (idx >= d) x = op(x, sh[cur][idx - d]);
    sh[cur ^ 1][idx] = x;
    cur ^= 1;
    __syncthreads();
  }
  return sh[cur];
}

// Length-limited Huffman code of freq[0..nsym): lens[], bit-reversed canonical codes[].  Called by the whole workgroup.
__device__ void build_code(const int* freq, int nsym, int maxbits, uint8_t* lens, uint16_t* codes, Huff& h) {
  const int tid = threadIdx.x;
  int f = 0;
  if (tid < nsym) {
    f = freq[tid];
    lens[tid] = 0;
    if (f > 0) {
      int r = 0;
      for (int j = 0; j < nsym; ++j) {
        const int fj = freq[j];
        r += (fj > 0 && (fj < f || (fj == f && j < tid))) ? 1 : 0;
      }
      h.sorted[r] = (uint16_t)tid;
    }
  }
  const int m = __syncthreads_count(f > 0);
  if (tid == 0) {
    for (int b = 0; b <= maxbits; ++b) h.count[b] = 0;
    if (m == 1) {
      h.count[1] = 1;
    } else if (m > 1) {
      int li = 0, ni = 0;
      for (int t = 0; t < m - 1; ++t) {
        int w = 0;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const int lw = li < m ? freq[h.sorted[li]] : 0;
          if (li < m && (ni >= t || lw <= h.nodew[ni])) {   // a leaf before an internal node of the same weight
            w += lw;
            h.leafpar[li++] = (uint16_t)t;
          } else {
            w += h.nodew[ni];
            h.nodepar[ni++] = (uint16_t)t;
          }
        }
        h.nodew[t] = w;
      }
      h.depth[m - 2] = 0;
      for (int k = m - 3; k >= 0; --k) h.depth[k] = (uint16_t)(h.depth[h.nodepar[k]] + 1);
      int kraft = 0;
      for (int a = 0; a < m; ++a) {
        const int d = min(h.depth[h.leafpar[a]] + 1, maxbits);
        h.count[d]++;
        kraft += 1 << (maxbits - d);
      }
      while (kraft > (1 << maxbits)) {   // zlib's repair: a leaf of the deepest level below the limit takes a sibling from the limit level
        int bits = maxbits - 1;
        while (h.count[bits] == 0) --bits;
        h.count[bits]--;
        h.count[bits + 1] += 2;
        h.count[maxbits]--;
        --kraft;
      }
    }
    int a = 0;
    for (int bits = maxbits; bits >= 1; --bits)
      for (int c = h.count[bits]; c > 0; --c) lens[h.sorted[a++]] = (uint8_t)bits;
    int code = 0;
    h.next[0] = 0;
    for (int bits = 1; bits <= maxbits; ++bits) {
      code = (code + (bits > 1 ? h.count[bits - 1] : 0)) << 1;
      h.next[bits] = code;
    }
  }
  __syncthreads();
  if (tid < nsym) {
    const int l = lens[tid];
    uint32_t c = 0;
    if (l > 0) {
      int before = 0;
      for (int j = 0; j < tid; ++j) before += lens[j] == l ? 1 : 0;
      c = __brev((uint32_t)(h.next[l] + before)) >> (32 - l);
    }
    codes[tid] = (uint16_t)c;
  }
  __syncthreads();
}

// length symbol of a match: index k into deflate's length table (symbol 257 + k), its extra-bit count and value
__device__ __forceinline__ void length_symbol(int len, int& k, int& eb, int& ev) {
  const int l = len - 3;
  if (len == 258) {
    k = 28, eb = 0, ev = 0;
  } else if (l < 8) {
    k = l, eb = 0, ev = 0;
  } else {
    eb = 29 - __clz(l);                 // floor(log2(l)) - 2
    k = 4 * eb + 4 + ((l >> eb) & 3);
    ev = l & ((1 << eb) - 1);
  }
}

// The tokens of positions [i0, i1) of the segment bytes s[0..n): f(position, match length or 0 for a literal).  q_in: start of the stretch
// that position i0 continues (last position <= i0 - 1 whose byte differs from the one before it, + 1); e_next: the first position >= i1
// whose byte differs from the one before it (n if none).
template <class F>
__device__ __forceinline__ void for_each_token(const uint8_t* s, int i0, int i1, int q_in, int e_next, F f) {
  int q = q_in, e = -1;
  for (int i = i0; i < i1; ++i) {
    const bool eq = i > 0 && s[i] == s[i - 1];
    if (!eq) {
      q = i + 1;
      e = -1;
      f(i, 0);
      continue;
    }
    if (e < 0) {   // first position of this chunk inside the stretch: find its end
      int j = i + 1;
      while (j < i1 && s[j] == s[j - 1]) ++j;
      e = j < i1 ? j : e_next;
    }
    const int j = i - q;
    const int k = j / 258;
    const int clen = min(258, (e - q) - 258 * k);
    if (clen < 3)
      f(i, 0);
    else if (j - 258 * k == 0)
      f(i, clen);
  }
}

__device__ __forceinline__ void or_bits(uint32_t* buf, int off, uint64_t v) {
  const int sh = off & 31, d = off >> 5;
  const uint64_t lo = v << sh;
  const uint32_t hi = sh ? (uint32_t)(v >> (64 - sh)) : 0u;
  if ((uint32_t)lo) atomicOr(&buf[d], (uint32_t)lo);
  if ((uint32_t)(lo >> 32)) atomicOr(&buf[d + 1], (uint32_t)(lo >> 32));
  if (hi) atomicOr(&buf[d + 2], hi);
}

// The compress stage both encoders share: the n <= kMaxSeg filtered bytes filt[] (LDS) -> one deflate block (+ the empty stored block of
// a non-final segment) in `slot`, its byte count in *nbytes, its Adler parts in adler_out[0..1].  bits: LDS of (n + 16 + 3) / 4 dwords
// that nobody reads any more (the bit buffer).  Called by the whole workgroup of kThreads behind a barrier that made filt[] visible.
// Its tables are static LDS of its own: a kernel that calls it adds them to its filtered bytes and its bit buffer.
__device__ __forceinline__ void compress_segment(uint32_t* bits, const uint8_t* filt, int n, bool final_seg, uint32_t* slot,
                                                 int32_t* nbytes, uint32_t* adler_out) {
  __shared__ int scan[2][kThreads];
  __shared__ int hist[kLit + 2];
  __shared__ uint8_t lens[kLit + 2];
  __shared__ uint16_t codes[kLit + 2];
  __shared__ int cl_hist[kClSyms];
  __shared__ uint8_t cl_lens[kClSyms + 1];
  __shared__ uint16_t cl_codes[kClSyms + 1];
  __shared__ uint16_t cl_tok[kMaxClTok];           // symbol | extra value << 5
  __shared__ Huff huff;
  __shared__ int sh_misc[8];                       // 0 matches, 1 nlit, 2 cl tokens, 3 header bits, 4 ncl
  __shared__ uint32_t sh_adler[2];
  const int tid = threadIdx.x;
  const int buf_dwords = (n + 16 + 3) / 4;
  for (int d = tid; d < buf_dwords; d += kThreads) bits[d] = 0;
  for (int i = tid; i < kLit + 2; i += kThreads) hist[i] = 0;
  if (tid < kClSyms) cl_hist[tid] = 0;
  if (tid < 8) sh_misc[tid] = 0;
  if (tid < 2) sh_adler[tid] = 0;
  __syncthreads();

  // ---- chunks, stretch scans, Adler parts
  const int P = (n + kThreads - 1) / kThreads;
  const int i0 = min(tid * P, n), i1 = min(i0 + P, n);
  int last_ne = -1, first_ne = n;
  uint32_t a1 = 0, a2 = 0;
  for (int i = i0; i < i1; ++i) {
    const uint32_t v = filt[i];
    a1 += v;
    a2 += (uint32_t)(n - i) * v;     // at most 49 terms below 2^23
    if (!(i > 0 && filt[i] == filt[i - 1])) {
      last_ne = i;
      if (first_ne == n) first_ne = i;
    }
  }
  atomicAdd(&sh_adler[0], a1 % kAdler);
  atomicAdd(&sh_adler[1], a2 % kAdler);
  const int* fw = block_scan(last_ne, tid, scan, [](int a, int b) { return max(a, b); });
  const int q_in = (tid > 0 ? fw[tid - 1] : -1) + 1;
  __syncthreads();
  const int* bw = block_scan(first_ne, kThreads - 1 - tid, scan, [](int a, int b) { return min(a, b); });
  const int e_next = tid < kThreads - 1 ? bw[kThreads - 2 - tid] : n;
  __syncthreads();

  // ---- histogram
  for_each_token(filt, i0, i1, q_in, e_next, [&](int i, int mlen) {
    if (mlen == 0) {
      atomicAdd(&hist[filt[i]], 1);
    } else {
      int k, eb, ev;
      length_symbol(mlen, k, eb, ev);
      atomicAdd(&hist[257 + k], 1);
      atomicAdd(&sh_misc[0], 1);
    }
  });
  if (tid == 0) hist[256] = 1;
  __syncthreads();
  build_code(hist, kLit, 15, lens, codes, huff);

  // ---- the code-length sequence in run-length form (one thread; at most 287 entries)
  if (tid == 0) {
    int nlit = kLit;
    while (nlit > 257 && lens[nlit - 1] == 0) --nlit;
    lens[kLit] = 0;
    const int dlen = sh_misc[0] > 0 ? 1 : 0;
    const int N = nlit + 1;
    auto at = [&](int i) { return i < nlit ? (int)lens[i] : dlen; };
    int nt = 0, i = 0;
    while (i < N) {
      const int v = at(i);
      int run = 1;
      while (i + run < N && at(i + run) == v) ++run;
      int sym, ev = 0, r = 1;
      if (v == 0) {
        if (run >= 11) {
          r = min(run, 138), sym = 18, ev = r - 11;
        } else if (run >= 3) {
          r = run, sym = 17, ev = r - 3;
        } else {
          sym = 0;
        }
      } else if (i > 0 && at(i - 1) == v && run >= 3) {
        r = min(run, 6), sym = 16, ev = r - 3;
      } else {
        sym = v;
      }
      cl_tok[nt++] = (uint16_t)(sym | ev << 5);
      cl_hist[sym]++;
      i += r;
    }
    sh_misc[1] = nlit;
    sh_misc[2] = nt;
  }
  __syncthreads();
  build_code(cl_hist, kClSyms, 7, cl_lens, cl_codes, huff);
  if (tid == 0) {
    int ncl = kClSyms;
    while (ncl > 4 && cl_lens[kClOrder[ncl - 1]] == 0) --ncl;
    int hb = 3 + 5 + 5 + 4 + 3 * ncl;
    const int nt = sh_misc[2];
    for (int t = 0; t < nt; ++t) {
      const int sym = cl_tok[t] & 31;
      hb += cl_lens[sym] + (sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0);
    }
    sh_misc[3] = hb;
    sh_misc[4] = ncl;
  }

  // ---- bit counts and their prefix sum
  int my_bits = 0;
  for_each_token(filt, i0, i1, q_in, e_next, [&](int i, int mlen) {
    if (mlen == 0) {
      my_bits += lens[filt[i]];
    } else {
      int k, eb, ev;
      length_symbol(mlen, k, eb, ev);
      my_bits += lens[257 + k] + eb + 1;
    }
  });
  const int* ps = block_scan(my_bits, tid, scan, [](int a, int b) { return a + b; });
  const int data_bits = ps[kThreads - 1];
  int off = sh_misc[3] + (tid > 0 ? ps[tid - 1] : 0);      // the scan's barriers made the header bit count visible
  const int hdr_bits = sh_misc[3];
  const int end_bits = hdr_bits + data_bits + lens[256];
  const int coded_total = final_seg ? (end_bits + 7) / 8 : (end_bits + 3 + 7) / 8 + 4;
  const int stored_total = 5 + n + (final_seg ? 0 : 5);
  const bool coded = coded_total < stored_total;
  const int total = coded ? coded_total : stored_total;
  uint8_t* bb = reinterpret_cast<uint8_t*>(bits);

  if (coded) {
    if (tid == 0) {   // the block header
      uint64_t acc = 0;
      int cnt = 0, d = 0;
      auto put = [&](uint32_t v, int nb) {
        acc |= (uint64_t)v << cnt;
        cnt += nb;
        if (cnt >= 32) {
          atomicOr(&bits[d++], (uint32_t)acc);
          acc >>= 32;
          cnt -= 32;
        }
      };
      const int ncl = sh_misc[4], nt = sh_misc[2];
      put(final_seg ? 1u : 0u, 1);
      put(2u, 2);
      put((uint32_t)(sh_misc[1] - 257), 5);
      put(0u, 5);
      put((uint32_t)(ncl - 4), 4);
      for (int k = 0; k < ncl; ++k) put(cl_lens[kClOrder[k]], 3);
      for (int t = 0; t < nt; ++t) {
        const int sym = cl_tok[t] & 31, ev = cl_tok[t] >> 5;
        const int cl = cl_lens[sym];
        put((uint32_t)cl_codes[sym] | (uint32_t)ev << cl, cl + (sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0));
      }
      if (cnt) atomicOr(&bits[d], (uint32_t)acc);
      or_bits(bits, hdr_bits + data_bits, codes[256]);
    }
    for_each_token(filt, i0, i1, q_in, e_next, [&](int i, int mlen) {
      if (mlen == 0) {
        const int s = filt[i];
        or_bits(bits, off, codes[s]);
        off += lens[s];
      } else {
        int k, eb, ev;
        length_symbol(mlen, k, eb, ev);
        const int l = lens[257 + k];
        or_bits(bits, off, (uint64_t)codes[257 + k] | (uint64_t)ev << l);   // the distance code (symbol 0) is one 0 bit behind them
        off += l + eb + 1;
      }
    });
    __syncthreads();
    if (!final_seg && tid == 0) {   // the empty stored block: its 3 header bits and the padding are zeros already
      bb[total - 2] = 0xFF;
      bb[total - 1] = 0xFF;
    }
  } else {
    if (tid == 0) {
      bb[0] = final_seg ? 1 : 0;
      bb[1] = (uint8_t)(n & 255);
      bb[2] = (uint8_t)(n >> 8);
      bb[3] = (uint8_t)(~n & 255);
      bb[4] = (uint8_t)((~n >> 8) & 255);
      if (!final_seg) bb[total - 2] = 0xFF, bb[total - 1] = 0xFF;
    }
    for (int i = tid; i < n; i += kThreads) bb[5 + i] = filt[i];
  }
  __syncthreads();

  // ---- store
  for (int d = tid; d * 4 < total; d += kThreads) slot[d] = bits[d];
  if (tid == 0) {
    *nbytes = total;
    adler_out[0] = sh_adler[0] % kAdler;
    adler_out[1] = sh_adler[1] % kAdler;
  }
}

__global__ __launch_bounds__(kThreads) void png_encode_kernel(uint8_t* out, int64_t out_capacity, int32_t* seg_bytes, uint32_t* seg_adler,
                                                              const uint8_t* src, int64_t src_bytes, int H, int W, int C) {
  __shared__ uint32_t rawd[kRawDwords];            // the raw rows; later the bit buffer
  __shared__ __align__(4) uint8_t filt[kMaxSeg + 4];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int seg = blockIdx.x, nseg = gridDim.x;
  const int64_t img = blockIdx.y;
  const int rb = C * W, L = rb + 1;
  const int r0 = seg * kRows;
  const int rows = min(kRows, H - r0);
  const int n = rows * L;
  const bool final_seg = seg == nseg - 1;

  // ---- load: rows fr .. r0 + rows - 1 as one byte range
  const int fr = max(r0 - 1, 0);
  const int nload = (r0 + rows - fr) * rb;
  const uintptr_t lo = (uintptr_t)src, hi = lo + (uintptr_t)src_bytes;
  const uintptr_t A = lo + (uintptr_t)((img * H + fr) * rb);
  const int mis = (int)(A & 3);
  for (int d = tid; d * 4 < mis + nload; d += kThreads) {
    const uintptr_t p = (A & ~(uintptr_t)3) + 4u * (uintptr_t)d;
    uint32_t v = 0;
    if (p >= lo && p + 4 <= hi) {
      v = *reinterpret_cast<const uint32_t*>(p);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (p + k >= lo && p + k < hi) v |= (uint32_t)(*reinterpret_cast<const uint8_t*>(p + k)) << (8 * k);
    }
    rawd[d] = v;
  }
  __syncthreads();

  // ---- filter: one wave per row
  const uint8_t* ls = reinterpret_cast<const uint8_t*>(rawd) + mis;
  for (int row = wave; row < rows; row += kWaves) {
    const int y = r0 + row;
    const uint8_t* cur = ls + (y - fr) * rb;
    const bool has_up = y > 0;
    int s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
    for (int x = lane; x < rb; x += 64) {
      const int v = cur[x];
      const int a = x >= C ? cur[x - C] : 0;
      const int b = has_up ? cur[x - rb] : 0;
      const int c = (has_up && x >= C) ? cur[x - rb - C] : 0;
      const int p = a + b - c;
      const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
      const int pr = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
      int r;
      r = v; s0 += r < 128 ? r : 256 - r;
      r = (v - a) & 255; s1 += r < 128 ? r : 256 - r;
      r = (v - b) & 255; s2 += r < 128 ? r : 256 - r;
      r = (v - ((a + b) >> 1)) & 255; s3 += r < 128 ? r : 256 - r;
      r = (v - pr) & 255; s4 += r < 128 ? r : 256 - r;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      s0 += __shfl_xor(s0, d, 64);
      s1 += __shfl_xor(s1, d, 64);
      s2 += __shfl_xor(s2, d, 64);
      s3 += __shfl_xor(s3, d, 64);
      s4 += __shfl_xor(s4, d, 64);
    }
    int type = 0, best = s0;
    if (s1 < best) type = 1, best = s1;
    if (s2 < best) type = 2, best = s2;
    if (s3 < best) type = 3, best = s3;
    if (s4 < best) type = 4, best = s4;
    uint8_t* o = filt + row * L;
    if (lane == 0) o[0] = (uint8_t)type;
    for (int x = lane; x < rb; x += 64) {
      const int v = cur[x];
      const int a = x >= C ? cur[x - C] : 0;
      const int b = has_up ? cur[x - rb] : 0;
      const int c = (has_up && x >= C) ? cur[x - rb - C] : 0;
      int pred = 0;
      if (type == 1) {
        pred = a;
      } else if (type == 2) {
        pred = b;
      } else if (type == 3) {
        pred = (a + b) >> 1;
      } else if (type == 4) {
        const int p = a + b - c;
        const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
        pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
      }
      o[1 + x] = (uint8_t)(v - pred);
    }
  }
  __syncthreads();

  // ---- the raw rows are done with: their LDS becomes the bit buffer
  const int64_t k = img * nseg + seg;
  compress_segment(rawd, filt, n, final_seg, reinterpret_cast<uint32_t*>(out + img * out_capacity + (int64_t)seg * seg_bound(kRows, rb)),
                   seg_bytes + k, seg_adler + 2 * k);
}

// ---------------------------------------------------------------------------------------------------------------- ragged batches
// Whole photos of any width, each with its own size inside one packed buffer: the filtered stream of an image is cut into segments of
// kRagSeg BYTES (a boundary may fall anywhere), so the LDS need does not depend on the row length.
//   png_row_filter_kernel      one workgroup per (image, row): the five sums straight from global memory -> the row's type byte
//   png_ragged_encode_kernel   one workgroup per (image, segment): the segment's filtered bytes rebuilt into LDS, compress_segment
//   png_compact_kernel         one workgroup per (image, segment): the slot -> its place in the image's contiguous payload
constexpr int kRagSeg = VSP_PNG_RAGGED_SEG_BYTES;
constexpr int kRagSlot = (kRagSeg + 10 + 3) / 4 * 4;
constexpr int kRowThreads = 256, kCopyThreads = 256;
static_assert(kRagSeg <= kMaxSeg && (kRagSeg + kThreads - 1) / kThreads <= 49, "compress_segment's chunks hold at most 49 bytes");
static_assert(kRagSlot == VSP_PNG_RAGGED_SLOT_BYTES, "the header's slot size");

__device__ __forceinline__ int paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ int abs8(int r) { return r < 128 ? r : 256 - r; }

// the last item whose `first` (seg0 or row0, ascending from 0) is <= j
template <class F>
__device__ __forceinline__ int find_image(int n, int j, F first) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (first(mid) <= j) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// segments of an image of h rows of L filtered bytes
__host__ __device__ inline int rag_segments(int h, int L) { return (int)(((int64_t)h * L + kRagSeg - 1) / kRagSeg); }

// grid (rows of the call), kRowThreads
__global__ __launch_bounds__(kRowThreads) void png_row_filter_kernel(uint8_t* __restrict__ types, const uint8_t* __restrict__ src,
                                                                     const vsp_png_item* __restrict__ items, int n, int C) {
  __shared__ int part[kRowThreads / 64][5];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = blockIdx.x;
  const vsp_png_item it = items[find_image(n, j, [&](int i) { return items[i].row0; })];
  const int y = j - it.row0;
  if (y < 0 || y >= it.h) return;
  const int rb = C * it.w;
  const uint8_t* cur = src + it.src_off + (int64_t)y * rb;
  const bool has_up = y > 0;
  int s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
  for (int x = tid; x < rb; x += kRowThreads) {
    const int v = cur[x];
    const int a = x >= C ? cur[x - C] : 0;
    const int b = has_up ? cur[x - rb] : 0;
    const int c = (has_up && x >= C) ? cur[x - rb - C] : 0;
    s0 += abs8(v);
    s1 += abs8((v - a) & 255);
    s2 += abs8((v - b) & 255);
    s3 += abs8((v - ((a + b) >> 1)) & 255);
    s4 += abs8((v - paeth(a, b, c)) & 255);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    s0 += __shfl_xor(s0, d, 64);
    s1 += __shfl_xor(s1, d, 64);
    s2 += __shfl_xor(s2, d, 64);
    s3 += __shfl_xor(s3, d, 64);
    s4 += __shfl_xor(s4, d, 64);
  }
  if (lane == 0) part[wave][0] = s0, part[wave][1] = s1, part[wave][2] = s2, part[wave][3] = s3, part[wave][4] = s4;
  __syncthreads();
  if (tid == 0) {
    int s[5];
    for (int k = 0; k < 5; ++k) {
      s[k] = 0;
      for (int w = 0; w < kRowThreads / 64; ++w) s[k] += part[w][k];
    }
    int type = 0, best = s[0];
    for (int k = 1; k < 5; ++k)
      if (s[k] < best) type = k, best = s[k];
    types[j] = (uint8_t)type;
  }
}

// grid (segments of the call), kThreads
__global__ __launch_bounds__(kThreads) void png_ragged_encode_kernel(uint8_t* __restrict__ slots, int32_t* __restrict__ seg_bytes,
                                                                     uint32_t* __restrict__ seg_adler, const uint8_t* __restrict__ types,
                                                                     const uint8_t* __restrict__ src, const vsp_png_item* __restrict__ items,
                                                                     int n_images, int C) {
  __shared__ uint32_t bits[(kRagSeg + 16 + 3) / 4];
  __shared__ __align__(4) uint8_t filt[kRagSeg + 4];
  const int tid = threadIdx.x;
  const int j = blockIdx.x;
  const vsp_png_item it = items[find_image(n_images, j, [&](int i) { return items[i].seg0; })];
  const int rb = C * it.w, L = rb + 1;
  const int li = j - it.seg0, nseg = rag_segments(it.h, L);
  if (li < 0 || li >= nseg) return;                 // cannot happen with a table the host has checked
  const int64_t total = (int64_t)it.h * L, p0 = (int64_t)li * kRagSeg;
  const int n = (int)min((int64_t)kRagSeg, total - p0);
  const int row0 = (int)(p0 / L), col0 = (int)(p0 - (int64_t)row0 * L);
  const uint8_t* img = src + it.src_off;
  const uint8_t* trow = types + it.row0;
  for (int i = tid; i < n; i += kThreads) {
    const uint32_t t = (uint32_t)(col0 + i);        // below kRagSeg + L
    const uint32_t dr = t / (uint32_t)L;
    const int col = (int)(t - dr * (uint32_t)L), y = row0 + (int)dr;
    const int type = trow[y];
    int r = type;
    if (col > 0) {
      const int x = col - 1;
      const uint8_t* cur = img + (int64_t)y * rb;
      const bool has_up = y > 0;
      const int v = cur[x];
      const int a = x >= C ? cur[x - C] : 0;
      const int b = has_up ? cur[x - rb] : 0;
      const int c = (has_up && x >= C) ? cur[x - rb - C] : 0;
      const int pred = type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : type == 4 ? paeth(a, b, c) : 0;
      r = v - pred;
    }
    filt[i] = (uint8_t)r;
  }
  __syncthreads();
  compress_segment(bits, filt, n, li == nseg - 1, reinterpret_cast<uint32_t*>(slots + (int64_t)j * kRagSlot), seg_bytes + j,
                   seg_adler + 2 * (int64_t)j);
}

// grid (segments of the call), kCopyThreads
__global__ __launch_bounds__(kCopyThreads) void png_compact_kernel(uint8_t* __restrict__ out, int32_t* __restrict__ idat_bytes,
                                                                   const uint8_t* __restrict__ slots, const int32_t* __restrict__ seg_bytes,
                                                                   const vsp_png_item* __restrict__ items, int n_images, int C) {
  __shared__ long long wsum[kCopyThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = blockIdx.x;
  const int im = find_image(n_images, j, [&](int i) { return items[i].seg0; });
  const vsp_png_item it = items[im];
  const int L = C * it.w + 1;
  const int li = j - it.seg0, nseg = rag_segments(it.h, L);
  if (li < 0 || li >= nseg) return;
  long long sum = 0;                                 // an image's payload can pass 2^31 by its 10 bytes per segment
  for (int k = tid; k < li; k += kCopyThreads) sum += min(max(seg_bytes[it.seg0 + k], 0), kRagSlot);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
  if (lane == 0) wsum[wave] = sum;
  __syncthreads();
  int64_t off = 0;
  for (int w = 0; w < kCopyThreads / 64; ++w) off += wsum[w];
  const int nb = min(max(seg_bytes[j], 0), kRagSlot);
  const int64_t bound = (int64_t)it.h * L + 10 * (int64_t)nseg;
  if (off + nb > bound) return;                      // cannot happen: every segment stays within its stored form
  const uint8_t* s = slots + (int64_t)j * kRagSlot;
  uint8_t* d = out + it.out_off + off;
  for (int i = tid; i < nb; i += kCopyThreads) d[i] = s[i];
  if (li == nseg - 1 && tid == 0) idat_bytes[im] = (int32_t)(off + nb);
}

constexpr size_t k2GiB = (size_t)1 << 31;

bool rag_size_ok(int H, int W, int C) {
  return H > 0 && W > 0 && (C == 1 || C == 3) && (int64_t)W * C <= VSP_PNG_RAGGED_MAX_ROW_BYTES && (uint64_t)H * W * C < k2GiB;
}

}  // namespace

extern "C" {

size_t vsp_png_segment_bound(int rows, int W, int C) {
  if (rows <= 0 || rows > VSP_PNG_SEG_ROWS || W <= 0 || (C != 1 && C != 3) || (int64_t)W * C > VSP_PNG_MAX_ROW_BYTES) return 0;
  return (size_t)seg_bound(rows, W * C);
}

size_t vsp_png_bound(int H, int W, int C) {
  if (H <= 0 || H > VSP_PNG_MAX_H || vsp_png_segment_bound(VSP_PNG_SEG_ROWS, W, C) == 0) return 0;
  return (size_t)((H + VSP_PNG_SEG_ROWS - 1) / VSP_PNG_SEG_ROWS) * vsp_png_segment_bound(VSP_PNG_SEG_ROWS, W, C);
}

int vsp_png_encode_u8(uint8_t* out, size_t out_capacity, int32_t* seg_bytes, uint32_t* seg_adler, const uint8_t* src, int B, int H, int W,
                      int C, vsp_stream_t stream) {
  VSP_REQUIRE(B >= 0 && H > 0 && W > 0, "png_encode: batch %d of %d x %d", B, H, W);
  VSP_REQUIRE(C == 1 || C == 3, "png_encode: %d channels (1 or 3)", C);
  if ((int64_t)W * C > VSP_PNG_MAX_ROW_BYTES || H > VSP_PNG_MAX_H || B > VSP_PNG_MAX_BATCH)
    return vsp::fail(VSP_ENOTSUP, "png_encode: %d x %d x %d, batch %d above the limits (row bytes %d, height %d, batch %d)", H, W, C, B,
                     VSP_PNG_MAX_ROW_BYTES, VSP_PNG_MAX_H, VSP_PNG_MAX_BATCH);
  if (B == 0) return VSP_OK;
  VSP_REQUIRE(out && seg_bytes && seg_adler && src, "png_encode: null pointer");
  VSP_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3u) == 0 && (out_capacity & 3u) == 0 && (reinterpret_cast<uintptr_t>(seg_bytes) & 3u) == 0 &&
                  (reinterpret_cast<uintptr_t>(seg_adler) & 3u) == 0,
              "png_encode: out, out_capacity, seg_bytes and seg_adler must be 4-byte aligned");
  VSP_REQUIRE(out_capacity >= vsp_png_bound(H, W, C), "png_encode: %zu bytes per image, vsp_png_bound asks for %zu", out_capacity,
              vsp_png_bound(H, W, C));
  const int nseg = (H + kRows - 1) / kRows;
  png_encode_kernel<<<dim3((unsigned)nseg, (unsigned)B), kThreads, 0, vsp::as_stream(stream)>>>(
      out, (int64_t)out_capacity, seg_bytes, seg_adler, src, (int64_t)B * H * W * C, H, W, C);
  return vsp::check_launch("png_encode");
}

int vsp_png_ragged_segments(int H, int W, int C) {
  if (!rag_size_ok(H, W, C)) return 0;
  return rag_segments(H, W * C + 1);
}

size_t vsp_png_ragged_image_bound(int H, int W, int C) {
  if (!rag_size_ok(H, W, C)) return 0;
  return (size_t)H * ((size_t)W * C + 1) + 10 * (size_t)rag_segments(H, W * C + 1);
}

size_t vsp_png_ragged_work_bytes(int64_t segments, int64_t rows) {
  if (segments < 0 || rows < 0) return 0;
  return (size_t)segments * (VSP_PNG_RAGGED_SLOT_BYTES + 4) + ((size_t)rows + 3) / 4 * 4;
}

int vsp_png_encode_ragged_u8(uint8_t* out, size_t out_bytes, int32_t* idat_bytes, uint32_t* seg_adler, uint8_t* work, size_t work_bytes,
                             const uint8_t* src, size_t src_bytes, const vsp_png_item* items, const vsp_png_item* items_dev, int n, int C,
                             vsp_stream_t stream) {
  VSP_REQUIRE(n >= 0, "png_encode_ragged: %d images", n);
  VSP_REQUIRE(C == 1 || C == 3, "png_encode_ragged: %d channels (1 or 3)", C);
  if (n > VSP_PNG_RAGGED_MAX_IMAGES) return vsp::fail(VSP_ENOTSUP, "png_encode_ragged: %d images (max %d)", n, VSP_PNG_RAGGED_MAX_IMAGES);
  if (n == 0) return VSP_OK;
  VSP_REQUIRE(out && idat_bytes && seg_adler && work && src && items && items_dev, "png_encode_ragged: null pointer");
  VSP_REQUIRE((reinterpret_cast<uintptr_t>(work) & 3u) == 0 && (reinterpret_cast<uintptr_t>(idat_bytes) & 3u) == 0 &&
                  (reinterpret_cast<uintptr_t>(seg_adler) & 3u) == 0,
              "png_encode_ragged: work, idat_bytes and seg_adler must be 4-byte aligned");
  if (src_bytes >= k2GiB || out_bytes >= k2GiB || work_bytes >= k2GiB)
    return vsp::fail(VSP_ENOTSUP, "png_encode_ragged: a buffer of 2 GiB or more (src %zu, out %zu, work %zu)", src_bytes, out_bytes, work_bytes);
  int64_t segs = 0, rows = 0, src_end = 0, out_end = 0;
  for (int i = 0; i < n; ++i) {
    const vsp_png_item& it = items[i];
    VSP_REQUIRE(it.h > 0 && it.w > 0, "png_encode_ragged: image %d is %d x %d", i, it.h, it.w);
    if ((int64_t)it.w * C > VSP_PNG_RAGGED_MAX_ROW_BYTES)
      return vsp::fail(VSP_ENOTSUP, "png_encode_ragged: image %d has rows of %lld bytes (max %d)", i, (long long)it.w * C,
                       VSP_PNG_RAGGED_MAX_ROW_BYTES);
    const uint64_t bytes = (uint64_t)it.h * it.w * C;
    VSP_REQUIRE(it.src_off >= src_end && (uint64_t)it.src_off + bytes <= src_bytes,
                "png_encode_ragged: image %d (offset %lld, %llu bytes) overlaps the image before it or leaves src (%zu bytes)", i,
                (long long)it.src_off, (unsigned long long)bytes, src_bytes);
    src_end = it.src_off + (int64_t)bytes;
    const int L = it.w * C + 1, nseg = rag_segments(it.h, L);
    const uint64_t bound = (uint64_t)it.h * L + 10 * (uint64_t)nseg;
    VSP_REQUIRE(it.out_off >= out_end && (uint64_t)it.out_off + bound <= out_bytes,
                "png_encode_ragged: the output range of image %d (offset %lld, %llu bytes) overlaps the one before it or leaves out (%zu bytes)",
                i, (long long)it.out_off, (unsigned long long)bound, out_bytes);
    out_end = it.out_off + (int64_t)bound;
    VSP_REQUIRE(it.seg0 == segs && it.row0 == rows, "png_encode_ragged: image %d has seg0 %d and row0 %d, expected %lld and %lld", i, it.seg0,
                it.row0, (long long)segs, (long long)rows);
    segs += nseg;
    rows += it.h;
    if (segs > VSP_PNG_RAGGED_MAX_SEGMENTS)
      return vsp::fail(VSP_ENOTSUP, "png_encode_ragged: more than %d segments in one call", VSP_PNG_RAGGED_MAX_SEGMENTS);
  }
  VSP_REQUIRE(vsp_png_ragged_work_bytes(segs, rows) <= work_bytes, "png_encode_ragged: work of %zu bytes, %lld segments and %lld rows need %zu",
              work_bytes, (long long)segs, (long long)rows, vsp_png_ragged_work_bytes(segs, rows));
  uint8_t* slots = work;
  int32_t* seg_bytes = reinterpret_cast<int32_t*>(work + (size_t)segs * VSP_PNG_RAGGED_SLOT_BYTES);
  uint8_t* types = work + (size_t)segs * (VSP_PNG_RAGGED_SLOT_BYTES + 4);
  hipStream_t s = vsp::as_stream(stream);
  png_row_filter_kernel<<<(unsigned)rows, kRowThreads, 0, s>>>(types, src, items_dev, n, C);
  int rc = vsp::check_launch("png_row_filter");
  if (rc != VSP_OK) return rc;
  png_ragged_encode_kernel<<<(unsigned)segs, kThreads, 0, s>>>(slots, seg_bytes, seg_adler, types, src, items_dev, n, C);
  rc = vsp::check_launch("png_ragged_encode");
  if (rc != VSP_OK) return rc;
  png_compact_kernel<<<(unsigned)segs, kCopyThreads, 0, s>>>(out, idat_bytes, slots, seg_bytes, items_dev, n, C);
  return vsp::check_launch("png_compact");
}

}  // extern "C"
