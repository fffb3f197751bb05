// Device-side baseline JPEG decoder for gfx950: a ragged batch of entropy-coded scans -> packed (h, w, 3) uint8 RGB images (format and
// rules in include/vspbfr_hip.h; the host restatement every byte is held to: tests/jpeg_dec_ref.py; the host parses the markers in front
// of the scan, vspbfr_amd/jpeg.py).  The pixels are those of libjpeg / libjpeg-turbo's default decode (ISLOW, fancy upsampling).
//
//   jpeg_dec_unstuff_kernel  one workgroup per image.  Pass A finds the first marker that is neither RSTm nor a stuffed / fill byte (the
//                            end of the scan); pass B is flag, scan, compact over 4096-byte chunks: the `00` behind a data `FF`, `FF`
//                            fill bytes and the RSTm markers are dropped, the clean bytes of all intervals go back to back into the
//                            item's work area and every RSTm leaves the clean offset of the interval behind it.
//   jpeg_dec_entropy_kernel  one workgroup per restart interval (1024 threads for an image that is one interval, 64 for the intervals of
//                            an image that has many).  The interval is cut into subsequences of sub_bytes; a lane decodes a subsequence
//                            from a given (bit position, block in MCU, zig-zag position) until it passes the subsequence's end and
//                            records its exit.  Round 0 starts every subsequence at its first bit in state (0, 0); in every later round
//                            subsequence i + 1 is decoded again from the exit of i recorded in the round before (two buffers, so the
//                            result does not depend on the order of the lanes) if that exit changed.  Subsequence 0 starts from the
//                            truth, so after r rounds the exits of 0 .. r are the truth: the loop ends when a round changed nothing, at
//                            the latest after as many rounds as there are subsequences.  Then a scan of the block counts gives every
//                            lane's contiguous run of subsequences its first block, and the true pass decodes once more and stores the
//                            coefficients (int16, natural order, DC as a difference) into the zeroed [block][64] buffer.
//   jpeg_dec_dc_kernel       one workgroup per interval: per component, the running sum of the DC differences
//   jpeg_dec_idct_kernel     one wave per MCU: dequantise, the two ISLOW passes + range limit (jpeg_common.h), samples to the planes
//   jpeg_dec_color_kernel    one thread per pixel: fancy h2v2 upsampling of the real chroma samples (4:2:0; plain 2 x 2 replication where
//                            the image has at most two chroma columns, as the library does) and YCbCr -> RGB
//
// The symbol loop is TOTAL: it runs on wrong states in every ordinary call.  A prefix that matches no code consumes one bit; a category
// above 11 (DC) / 10 (AC) consumes its bits like any other; a run that carries k past 63 ends the block.  Every iteration consumes at
// least one bit and the loop ends when the bit position passes the subsequence's end; bytes are loaded through one function that clamps
// to the interval (bits past its end read as 1); blocks past the interval's expected count are not stored.  In the true pass these
// events, and a block count other than the expected one, are ORed into the image's status word.
#include "vsp_common.h"
#include "jpeg_common.h"

namespace {

using namespace vsp_jpeg;

constexpr int kTableBytes = VSP_JPEG_DEC_TABLE_BYTES;   // per image: 3 x 64 quantisers (natural order), 6 x (16 BITS + 256 HUFFVAL)
constexpr int kHuffBytes = 272;
constexpr int kMaxSubBytes = 4096;
constexpr size_t k2GiB = (size_t)1 << 31;

// zig-zag position -> natural order
__host__ __device__ inline int natural_of(int k) {
  constexpr unsigned char z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return z[k & 63];
}

// where an image's pieces lie in its work area (byte offsets from work_off, each a multiple of 16)
struct DecLayout {
  int m, mw, mh, mcus, bpm, nint, nblocks, cap, ph, pw;
  int64_t clean, ivl, ex, chg, coef, planes, total;
};

__host__ __device__ inline int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }

__host__ __device__ inline DecLayout dec_layout(int h, int w, int in_len, int sub, int restart, int sb) {
  DecLayout L;
  L.m = sub == VSP_JPEG_420 ? 16 : 8;
  L.bpm = sub == VSP_JPEG_420 ? 6 : 3;
  L.mw = (w + L.m - 1) / L.m, L.mh = (h + L.m - 1) / L.m;
  L.mcus = L.mw * L.mh;
  L.nint = restart > 0 ? (L.mcus + restart - 1) / restart : 1;
  L.nblocks = L.mcus * L.bpm;
  L.cap = in_len / sb + L.nint + 1;           // subsequence slots: interval i's first is (its clean offset) / sb + i
  L.ph = L.mh * L.m, L.pw = L.mw * L.m;
  L.clean = 0;
  L.ivl = up16((int64_t)in_len + 8);
  L.ex = L.ivl + up16(((int64_t)L.nint + 1) * 4);
  L.chg = L.ex + (int64_t)L.cap * 32;         // two buffers of int4 (bit position, state, blocks completed, 0)
  L.coef = L.chg + up16((int64_t)L.cap * 2);
  L.planes = L.coef + (int64_t)L.nblocks * 128;
  const int64_t pl = (int64_t)L.ph * L.pw;
  L.total = up16(L.planes + (sub == VSP_JPEG_420 ? pl + pl / 2 : 3 * pl));
  return L;
}

__host__ __device__ inline DecLayout dec_layout(const vsp_jpeg_dec_item& it, int sb) {
  return dec_layout(it.h, it.w, it.in_len, it.subsampling, it.restart, sb);
}

__host__ __device__ inline int block_comp(int bpm, int b) { return bpm == 6 ? (b < 4 ? 0 : b - 3) : b; }

// the item that owns global interval j: interval0 ascends strictly (checked on the host)
__device__ inline int find_item(const vsp_jpeg_dec_item* items, int n, int j) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (items[mid].interval0 <= j) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ int wave_scan_incl(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

// inclusive scan of one int per thread over a workgroup of T threads (T a multiple of 64, at most 1024); wsum: T / 64 ints of LDS
template <int T>
__device__ inline int block_scan_incl(int v, int* wsum, int t, int& total) {
  const int lane = t & 63, wv = t >> 6;
  int incl = wave_scan_incl(v, lane);
  __syncthreads();                             // wsum may still be read from the call before
  if (lane == 63) wsum[wv] = incl;
  __syncthreads();
  int before = 0, all = 0;
  for (int i = 0; i < T / 64; ++i) {
    const int s = wsum[i];
    if (i < wv) before += s;
    all += s;
  }
  total = all;
  return incl + before;
}

// ------------------------------------------------------------------------------------------------------------ unstuff and split
// grid (n), 256 threads
__global__ __launch_bounds__(256) void jpeg_dec_unstuff_kernel(const uint8_t* __restrict__ in, const vsp_jpeg_dec_item* __restrict__ items,
                                                                uint8_t* __restrict__ work, int32_t* __restrict__ status, int sb) {
  __shared__ int s_end;
  __shared__ int wsum[4];
  const vsp_jpeg_dec_item it = items[blockIdx.x];
  const DecLayout L = dec_layout(it, sb);
  const uint8_t* src = in + it.in_off;
  const int len = it.in_len, t = threadIdx.x;
  uint8_t* clean = work + it.work_off + L.clean;
  int32_t* ivl = reinterpret_cast<int32_t*>(work + it.work_off + L.ivl);
  int err = 0;
  if (t == 0) s_end = len;
  __syncthreads();
  for (int p = t; p + 1 < len; p += 256)
    if (src[p] == 0xFF) {
      const int nx = src[p + 1];
      if (nx != 0 && nx != 0xFF && (nx & 0xF8) != 0xD0) atomicMin(&s_end, p);
    }
  __syncthreads();
  const int E = s_end;
  if (t == 0) err |= E == len ? VSP_JPEG_DEC_NO_EOI : (src[E + 1] != 0xD9 ? VSP_JPEG_DEC_STRAY_MARKER : 0);
  int run_keep = 0, run_mark = 0;
  for (int base = 0; base < E; base += 4096) {
    const int j0 = base + t * 16;
    unsigned keepm = 0, markm = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int j = j0 + q;
      if (j < E) {
        const int b = src[j], prev = j > 0 ? src[j - 1] : 0, nxt = j + 1 < len ? src[j + 1] : 0xD9;
        if (b == 0xFF ? nxt == 0 : prev != 0xFF) keepm |= 1u << q;
        if (b == 0xFF && (nxt & 0xF8) == 0xD0) markm |= 1u << q;
      }
    }
    const int packed = (__popc(markm) << 16) | __popc(keepm);
    int total;
    const int incl = block_scan_incl<256>(packed, wsum, t, total);
    int ko = run_keep + ((incl - packed) & 0xFFFF), mo = run_mark + ((incl - packed) >> 16);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      if (keepm >> q & 1u) {
        if (ko < len) clean[ko] = src[j0 + q];
        ++ko;
      }
      if (markm >> q & 1u) {
        ++mo;                                  // the interval this marker opens
        if (mo < L.nint) ivl[mo] = ko;
        if ((src[j0 + q + 1] & 7) != ((mo - 1) & 7)) err |= VSP_JPEG_DEC_RST_ORDER;
      }
    }
    run_keep += total & 0xFFFF, run_mark += total >> 16;
  }
  if (run_mark != L.nint - 1) err |= VSP_JPEG_DEC_RST_COUNT;
  const int kept = min(run_keep, len);
  for (int i = min(run_mark, L.nint - 1) + 1 + t; i <= L.nint; i += 256) ivl[i] = kept;
  if (t == 0) ivl[0] = 0;
  if (err) atomicOr(&status[blockIdx.x], err);
}

// ---------------------------------------------------------------------------------------------------------------- entropy decode
struct Huff {
  uint16_t look[512];    // 9-bit prefix -> length << 8 | symbol; 0: longer than 9 bits, or no code
  int32_t maxcode[17];   // [length] the largest code of that length, -1 without one
  int32_t valoff[17];    // [length] index in val of the first code of that length, minus that code
  uint8_t val[256];
};

// one thread: BITS / HUFFVAL -> the table.  look is zeroed by the caller.  The host checked that the counts fit 256 symbols and the code
// space; the indices are masked all the same.
__host__ __device__ inline void build_huff(Huff& h, const uint8_t* spec) {
  int code = 0, k = 0;
  for (int len = 1; len <= 16; ++len) {
    const int cnt = spec[len - 1];
    h.valoff[len] = k - code;
    h.maxcode[len] = cnt ? code + cnt - 1 : -1;
    for (int i = 0; i < cnt; ++i, ++code, ++k)
      if (len <= 9) {
        const uint16_t e = (uint16_t)(len << 8 | spec[16 + (k & 255)]);
        const int first = code << (9 - len);
        for (int f = 0; f < (1 << (9 - len)); ++f) h.look[(first + f) & 511] = e;
      }
    code <<= 1;
  }
  h.maxcode[0] = -1, h.valoff[0] = 0;
  for (int i = 0; i < 256; ++i) h.val[i] = spec[16 + i];
}

// MSB-first reader over the clean bytes of one interval; bits past its end read as 1
struct BitReader {
  const uint8_t* p;
  int len, next, cnt;
  uint64_t buf;
  __host__ __device__ __forceinline__ void init(const uint8_t* bytes, int nbytes, int pos) {
    p = bytes, len = nbytes, next = pos >> 3, cnt = 0, buf = 0;
    fill();
    skip(pos & 7);
  }
  __host__ __device__ __forceinline__ void fill() {
    while (cnt <= 56) {
      const uint64_t b = next >= 0 && next < len ? p[next] : 0xFFu;
      buf |= b << (56 - cnt);
      cnt += 8, ++next;
    }
  }
  __host__ __device__ __forceinline__ uint32_t peek(int n) const { return n ? (uint32_t)(buf >> (64 - n)) : 0u; }   // n <= 32
  __host__ __device__ __forceinline__ void skip(int n) { buf <<= n, cnt -= n; }
};

struct Exit {
  int pos, state, nblk;
};

// Decode from bit `pos` in state (block in MCU << 8 | zig-zag position) until the position reaches end_bit.  `last`: the subsequence is
// the interval's last, where up to 7 padding 1-bits behind a whole MCU end the data.  kStore: the true pass.
template <bool kStore>
__host__ __device__ inline Exit decode_sub(const Huff* huff, int bpm, const uint8_t* bytes, int nbytes, int pos, int state, int end_bit, bool last,
                                  int16_t* coef, int blk, int blk_end, int& err) {
  int b = state >> 8, k = state & 255, nblk = 0;
  BitReader br;
  br.init(bytes, nbytes, pos);
  while (pos < end_bit) {
    br.fill();
    const int left = end_bit - pos;
    if (last && state == 0 && left < 8 && br.peek(left) == (1u << left) - 1u) {
      pos = end_bit;
      break;
    }
    const Huff& h = huff[block_comp(bpm, b) * 2 + (k ? 1 : 0)];
    const uint32_t p16 = br.peek(16);
    int clen = 0, sym = 0;
    const uint32_t e = h.look[p16 >> 7];
    if (e) {
      clen = (int)(e >> 8), sym = (int)(e & 255u);
    } else {
      for (int l = 10; l <= 16; ++l) {
        const int code = (int)(p16 >> (16 - l));
        if (code <= h.maxcode[l]) {
          clen = l, sym = h.val[(code + h.valoff[l]) & 255];
          break;
        }
      }
    }
    if (clen == 0) {                            // no code has this prefix
      err |= VSP_JPEG_DEC_BAD_CODE;
      br.skip(1), pos += 1;
      continue;
    }
    br.skip(clen);
    const int s = sym & 15, r = sym >> 4;
    const int raw = (int)br.peek(s);
    br.skip(s);
    pos += clen + s;
    const int value = s && raw < (1 << (s - 1)) ? raw - (1 << s) + 1 : raw;
    if (k == 0) {
      if (sym > 11) err |= VSP_JPEG_DEC_BAD_CATEGORY;
      if (kStore && blk < blk_end) coef[(int64_t)blk * 64] = (int16_t)value;
      k = 1;
    } else if (s == 0) {
      if (r == 15) {                            // ZRL
        k += 16;
        if (k > 63) err |= VSP_JPEG_DEC_RUN, k = 64;
      } else {                                  // EOB; a run length with it belongs to progressive scans
        if (r) err |= VSP_JPEG_DEC_RUN;
        k = 64;
      }
    } else {
      if (s > 10) err |= VSP_JPEG_DEC_BAD_CATEGORY;
      k += r;
      if (k > 63) {
        err |= VSP_JPEG_DEC_RUN, k = 64;
      } else {
        if (kStore && blk < blk_end) coef[(int64_t)blk * 64 + natural_of(k)] = (int16_t)value;
        ++k;
      }
    }
    if (k >= 64) {
      k = 0, b = b + 1 == bpm ? 0 : b + 1;
      ++nblk, ++blk;
    }
    state = b << 8 | k;
  }
  return Exit{pos, b << 8 | k, nblk};
}

// kSingle: grid (n), the images that are one interval; otherwise grid (intervals of the call), the intervals of the other images
template <int T, bool kSingle>
__global__ __launch_bounds__(T) void jpeg_dec_entropy_kernel(const vsp_jpeg_dec_item* __restrict__ items, int n, const uint8_t* __restrict__ tables,
                                                              uint8_t* work, int32_t* __restrict__ status, int32_t* __restrict__ rounds, int sb) {
  __shared__ Huff huff[6];
  __shared__ int wsum[T / 64];
  __shared__ int s_min, s_max;
  const int t = threadIdx.x;
  const int idx = kSingle ? (int)blockIdx.x : find_item(items, n, blockIdx.x);
  const vsp_jpeg_dec_item it = items[idx];
  const DecLayout L = dec_layout(it, sb);
  const int li = kSingle ? 0 : (int)blockIdx.x - it.interval0;
  if ((L.nint == 1) != kSingle || li < 0 || li >= L.nint) return;
  uint8_t* base = work + it.work_off;
  const int32_t* ivl = reinterpret_cast<const int32_t*>(base + L.ivl);
  const int s0 = min(max(ivl[li], 0), it.in_len), s1 = min(max(ivl[li + 1], s0), it.in_len);
  const uint8_t* bytes = base + L.clean + s0;
  const int len = s1 - s0;
  const int sub0 = s0 / sb + li;
  const int nsub = min((len + sb - 1) / sb, L.cap - sub0);
  for (int i = t; i < 6 * 512; i += T) huff[i >> 9].look[i & 511] = 0;
  __syncthreads();
  if (t < 6) build_huff(huff[t], tables + (int64_t)idx * kTableBytes + 192 + t * kHuffBytes);
  __syncthreads();
  const int mcus_in = it.restart > 0 ? min(it.restart, L.mcus - li * it.restart) : L.mcus;
  const int blk0 = li * (it.restart > 0 ? it.restart : 0) * L.bpm, blk_end = blk0 + mcus_in * L.bpm;
  if (nsub <= 0) {
    if (t == 0) atomicOr(&status[idx], VSP_JPEG_DEC_BLOCK_COUNT);
    return;
  }
  int4* ex0 = reinterpret_cast<int4*>(base + L.ex) + sub0;     // buffer c of the exits: ex0 + c * cap
  uint8_t* chg0 = base + L.chg + sub0;                           // "this exit changed in the round that wrote it"
  auto ex = [&](int c) { return ex0 + (int64_t)c * L.cap; };
  auto chg = [&](int c) { return chg0 + (int64_t)c * L.cap; };
  int16_t* coef = reinterpret_cast<int16_t*>(base + L.coef);
  int err = 0;
  auto end_of = [&](int i) { return min((i + 1) * sb, len) * 8; };
  for (int i = t; i < nsub; i += T) {
    const Exit e = decode_sub<false>(huff, L.bpm, bytes, len, i * sb * 8, 0, end_of(i), i == nsub - 1, nullptr, 0, 0, err);
    ex(0)[i] = make_int4(e.pos, e.state, e.nblk, 0);
    chg(0)[i] = 1;
  }
  __syncthreads();
  // Round r decodes D_r = (the subsequences behind an exit that round r - 1 changed) and walks the hull of D_r and D_(r-1): what round
  // r - 1 decoded and round r does not is copied, so that outside the two ranges both buffers hold the latest exit.
  int cur = 0, r = 1;
  int dlo = 1, dhi = nsub - 1, ilo = 0, ihi = nsub - 1;
  while (nsub > 1 && r <= nsub) {              // after round r the exits of subsequences 0 .. r are the truth
    if (t == 0) s_min = 0x7FFFFFFF, s_max = -1;
    __syncthreads();
    int mn = 0x7FFFFFFF, mx = -1;
    for (int i = ilo + t; i <= ihi; i += T) {
      int4 mine = ex(cur)[i];
      int c = 0;
      if (i >= dlo && i <= dhi && chg(cur)[i - 1]) {
        const int4 from = ex(cur)[i - 1];
        const Exit e = decode_sub<false>(huff, L.bpm, bytes, len, from.x, from.y, end_of(i), i == nsub - 1, nullptr, 0, 0, err);
        c = e.pos != mine.x || e.state != mine.y || e.nblk != mine.z;
        mine = make_int4(e.pos, e.state, e.nblk, 0);
      }
      ex(cur ^ 1)[i] = mine;
      chg(cur ^ 1)[i] = (uint8_t)c;
      if (c) mn = min(mn, i), mx = max(mx, i);
    }
    if (mx >= 0) atomicMin(&s_min, mn), atomicMax(&s_max, mx);
    cur ^= 1, ++r;
    __syncthreads();
    const int gmin = s_min, gmax = s_max;
    __syncthreads();
    if (gmax < 0) break;
    const int nlo = gmin + 1, nhi = min(gmax + 1, nsub - 1);
    ilo = min(dlo, nlo), ihi = max(dhi, nhi);
    dlo = nlo, dhi = nhi;
  }
  __syncthreads();
  // every lane takes a contiguous run of subsequences; a scan of the runs' block counts gives each its first block
  const int per = (nsub + T - 1) / T, i0 = min(t * per, nsub), i1 = min(i0 + per, nsub);
  int mine = 0;
  for (int i = i0; i < i1; ++i) mine += ex(cur)[i].z;
  int total;
  const int incl = block_scan_incl<T>(mine, wsum, t, total);
  int blk = blk0 + incl - mine;
  err = 0;
  for (int i = i0; i < i1; ++i) {
    const int4 from = i ? ex(cur)[i - 1] : make_int4(0, 0, 0, 0);
    const Exit e = decode_sub<true>(huff, L.bpm, bytes, len, from.x, from.y, end_of(i), i == nsub - 1, coef, blk, blk_end, err);
    blk += e.nblk;
    if (i == nsub - 1 && (blk != blk_end || e.state != 0 || e.pos != len * 8)) err |= VSP_JPEG_DEC_BLOCK_COUNT;
  }
  if (err) atomicOr(&status[idx], err);
  if (t == 0 && rounds) atomicMax(&rounds[idx], r);
}

// ------------------------------------------------------------------------------------------------------------------------ DC
// grid (intervals of the call), 256 threads: each lane takes a contiguous run of the interval's MCUs
__global__ __launch_bounds__(256) void jpeg_dec_dc_kernel(const vsp_jpeg_dec_item* __restrict__ items, int n, uint8_t* work, int sb) {
  __shared__ int wsum[4];
  const int t = threadIdx.x;
  const int idx = find_item(items, n, blockIdx.x);
  const vsp_jpeg_dec_item it = items[idx];
  const DecLayout L = dec_layout(it, sb);
  const int li = (int)blockIdx.x - it.interval0;
  if (li < 0 || li >= L.nint) return;
  const int m0 = it.restart > 0 ? li * it.restart : 0, mcus_in = it.restart > 0 ? min(it.restart, L.mcus - m0) : L.mcus;
  int16_t* coef = reinterpret_cast<int16_t*>(work + it.work_off + L.coef);
  const int per = (mcus_in + 255) / 256, a = min(t * per, mcus_in), z = min(a + per, mcus_in);
  int sum[3] = {0, 0, 0};
  for (int m = a; m < z; ++m)
    for (int b = 0; b < L.bpm; ++b) {
      const int v = coef[((int64_t)(m0 + m) * L.bpm + b) * 64];
      const int c = block_comp(L.bpm, b);
      sum[0] += c == 0 ? v : 0, sum[1] += c == 1 ? v : 0, sum[2] += c == 2 ? v : 0;
    }
  int pred[3], total;
#pragma unroll
  for (int c = 0; c < 3; ++c) pred[c] = block_scan_incl<256>(sum[c], wsum, t, total) - sum[c];
  for (int m = a; m < z; ++m)
    for (int b = 0; b < L.bpm; ++b) {
      int16_t* d = coef + ((int64_t)(m0 + m) * L.bpm + b) * 64;
      const int c = block_comp(L.bpm, b), v = *d;
      const int now = (c == 0 ? pred[0] : c == 1 ? pred[1] : pred[2]) + v;
      pred[0] = c == 0 ? now : pred[0], pred[1] = c == 1 ? now : pred[1], pred[2] = c == 2 ? now : pred[2];
      *d = (int16_t)now;
    }
}

// ---------------------------------------------------------------------------------------------------------------------- pixels
// grid (largest MCU count, n), 64 threads: one MCU.  Planes: Y (ph x pw), then Cb and Cr (4:2:0: ph/2 x pw/2; 4:4:4: ph x pw)
__global__ __launch_bounds__(64) void jpeg_dec_idct_kernel(const vsp_jpeg_dec_item* __restrict__ items, const uint8_t* __restrict__ tables,
                                                            uint8_t* __restrict__ work, int32_t* __restrict__ status, int sb) {
  __shared__ int blk[6][64];
  __shared__ int qt[3][64];
  const vsp_jpeg_dec_item it = items[blockIdx.y];
  const DecLayout L = dec_layout(it, sb);
  const int m = blockIdx.x, t = threadIdx.x;
  if (m >= L.mcus) return;
  const uint8_t* q = tables + (int64_t)blockIdx.y * kTableBytes;
  for (int c = 0; c < 3; ++c) qt[c][t] = q[c * 64 + t];
  const int16_t* coef = reinterpret_cast<const int16_t*>(work + it.work_off + L.coef) + (int64_t)m * L.bpm * 64;
  bool wide = false;
  for (int b = 0; b < L.bpm; ++b) {
    const int v = coef[b * 64 + t] * qt[block_comp(L.bpm, b)][t];
    wide |= v > VSP_JPEG_DEC_COEF_LIMIT || v < -VSP_JPEG_DEC_COEF_LIMIT;
    blk[b][t] = v;
  }
  if (wide) atomicOr(&status[blockIdx.y], VSP_JPEG_DEC_COEF_RANGE);
  __syncthreads();
  const int b8 = t >> 3, v8 = t & 7;
  if (t < L.bpm * 8) idct8<false>(&blk[b8][v8], 8);
  __syncthreads();
  if (t < L.bpm * 8) idct8<true>(&blk[b8][v8 * 8], 1);
  __syncthreads();
  const int my = m / L.mw, mx = m - my * L.mw;
  uint8_t* yp = work + it.work_off + L.planes;
  const int64_t pl = (int64_t)L.ph * L.pw;
  if (L.bpm == 6) {
    for (int b = 0; b < 4; ++b) {
      const int yy = (b >> 1) * 8 + (t >> 3), xx = (b & 1) * 8 + (t & 7);
      yp[(int64_t)(my * 16 + yy) * L.pw + mx * 16 + xx] = (uint8_t)blk[b][t];
    }
    const int64_t co = (int64_t)(my * 8 + (t >> 3)) * (L.pw / 2) + mx * 8 + (t & 7);
    yp[pl + co] = (uint8_t)blk[4][t];
    yp[pl + pl / 4 + co] = (uint8_t)blk[5][t];
  } else {
    const int64_t o = (int64_t)(my * 8 + (t >> 3)) * L.pw + mx * 8 + (t & 7);
    for (int c = 0; c < 3; ++c) yp[c * pl + o] = (uint8_t)blk[c][t];
  }
}

// grid (ceil(largest pixel count / 256), n), 256 threads
__global__ __launch_bounds__(256) void jpeg_dec_color_kernel(uint8_t* __restrict__ out, const vsp_jpeg_dec_item* __restrict__ items,
                                                              const uint8_t* __restrict__ work, int sb) {
  const vsp_jpeg_dec_item it = items[blockIdx.y];
  const DecLayout L = dec_layout(it, sb);
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (int64_t)it.h * it.w) return;
  const int y = (int)(p / it.w), x = (int)(p - (int64_t)y * it.w);
  const uint8_t* yp = work + it.work_off + L.planes;
  const int64_t pl = (int64_t)L.ph * L.pw;
  const int Y = yp[(int64_t)y * L.pw + x];
  int Cb, Cr;
  if (L.bpm == 6) {
    const JpegGeom g = jpeg_geom(it.h, it.w);
    const uint8_t* cb = yp + pl;
    const uint8_t* cr = cb + pl / 4;
    const int cpw = L.pw / 2;
    if (g.cw > 2) {
      Cb = fancy_h2v2(g, y, x, [&](int r, int c) -> int { return cb[(int64_t)r * cpw + c]; });
      Cr = fancy_h2v2(g, y, x, [&](int r, int c) -> int { return cr[(int64_t)r * cpw + c]; });
    } else {   // jdsample.c takes the fancy filter only for more than two chroma columns; below that every sample is replicated 2 x 2
      Cb = cb[(int64_t)(y >> 1) * cpw + (x >> 1)];
      Cr = cr[(int64_t)(y >> 1) * cpw + (x >> 1)];
    }
  } else {
    Cb = yp[pl + (int64_t)y * L.pw + x];
    Cr = yp[2 * pl + (int64_t)y * L.pw + x];
  }
  int R, G, B;
  ycc_rgb(Y, Cb, Cr, R, G, B);
  uint8_t* o = out + it.out_off + p * 3;
  o[0] = (uint8_t)R, o[1] = (uint8_t)G, o[2] = (uint8_t)B;
}

bool sub_ok(int sub) { return sub == VSP_JPEG_444 || sub == VSP_JPEG_420; }
bool sub_bytes_ok(int sb) { return sb >= 4 && sb <= kMaxSubBytes && sb % 4 == 0; }

}  // namespace

extern "C" {

size_t vsp_jpeg_decode_work_bytes(int h, int w, int in_len, int subsampling, int restart, int sub_bytes) {
  if (h < 1 || h > 65535 || w < 1 || w > 65535 || in_len < 1 || in_len > VSP_JPEG_DEC_MAX_SCAN_BYTES || !sub_ok(subsampling) || restart < 0 ||
      restart > 65535 || !sub_bytes_ok(sub_bytes))
    return 0;
  return (size_t)dec_layout(h, w, in_len, subsampling, restart, sub_bytes).total;
}

int vsp_jpeg_decode_u8(uint8_t* out, size_t out_bytes, int32_t* status, int32_t* rounds, uint8_t* work, size_t work_bytes, const uint8_t* in,
                       size_t in_bytes, const vsp_jpeg_dec_item* items, const vsp_jpeg_dec_item* items_dev, const uint8_t* tables,
                       const uint8_t* tables_dev, int n, int sub_bytes, vsp_stream_t stream) {
  VSP_REQUIRE(n >= 0 && n <= VSP_JPEG_MAX_ITEMS, "jpeg_decode: %d items (max %d)", n, VSP_JPEG_MAX_ITEMS);
  VSP_REQUIRE(sub_bytes_ok(sub_bytes), "jpeg_decode: sub_bytes %d (a multiple of 4 in 4..%d)", sub_bytes, kMaxSubBytes);
  if (n == 0) return VSP_OK;
  VSP_REQUIRE(out && status && work && in && items && items_dev && tables && tables_dev, "jpeg_decode: null pointer");
  VSP_REQUIRE(vsp::aligned16(work), "jpeg_decode: work is not 16-byte aligned");
  if (in_bytes >= k2GiB || out_bytes >= k2GiB || work_bytes >= k2GiB)
    return vsp::fail(VSP_ENOTSUP, "jpeg_decode: a buffer of 2 GiB or more (in %zu, out %zu, work %zu)", in_bytes, out_bytes, work_bytes);
  int64_t intervals = 0, need = 0, max_pixels = 0, out_end = 0;
  int max_mcus = 0, singles = 0;
  for (int i = 0; i < n; ++i) {
    const vsp_jpeg_dec_item& it = items[i];
    VSP_REQUIRE(it.h >= 1 && it.h <= 65535 && it.w >= 1 && it.w <= 65535, "jpeg_decode: item %d is %d x %d (1..65535)", i, it.h, it.w);
    VSP_REQUIRE(sub_ok(it.subsampling), "jpeg_decode: item %d has subsampling %d (VSP_JPEG_444 or VSP_JPEG_420)", i, it.subsampling);
    VSP_REQUIRE(it.restart >= 0 && it.restart <= 65535, "jpeg_decode: item %d has restart interval %d outside 0..65535", i, it.restart);
    VSP_REQUIRE(it.in_len >= 1 && it.in_len <= VSP_JPEG_DEC_MAX_SCAN_BYTES, "jpeg_decode: item %d has a scan of %d bytes (1..%d)", i, it.in_len,
                VSP_JPEG_DEC_MAX_SCAN_BYTES);
    VSP_REQUIRE(it.in_off >= 0 && (uint64_t)it.in_off + (uint64_t)it.in_len <= in_bytes, "jpeg_decode: item %d lies outside in", i);
    VSP_REQUIRE(it.out_off >= 0 && (uint64_t)it.out_off + (uint64_t)it.h * it.w * 3 <= out_bytes, "jpeg_decode: item %d lies outside out", i);
    VSP_REQUIRE(it.out_off >= out_end, "jpeg_decode: item %d overlaps the image before it in out (out_off must ascend)", i);
    out_end = it.out_off + (int64_t)it.h * it.w * 3;
    VSP_REQUIRE(it.interval0 == intervals, "jpeg_decode: item %d has interval0 %d, expected %lld", i, it.interval0, (long long)intervals);
    VSP_REQUIRE(it.work_off == need, "jpeg_decode: item %d has work_off %lld, expected %lld", i, (long long)it.work_off, (long long)need);
    for (int k = 0; k < 6; ++k) {
      const uint8_t* bits = tables + (size_t)i * kTableBytes + 192 + k * kHuffBytes;
      int count = 0, code = 0;
      bool fits = true;
      for (int len = 1; len <= 16; ++len) {
        count += bits[len - 1], code += bits[len - 1];
        fits &= code < (1 << len);               // == : the all-ones code is in use, which the padding of an interval must not be
        code <<= 1;
      }
      VSP_REQUIRE(count <= 256 && fits, "jpeg_decode: Huffman table %d of item %d has %d codes%s", k, i, count,
                  fits ? "" : " and fills or overfills the code space (the all-ones code must stay free)");
    }
    const DecLayout L = dec_layout(it, sub_bytes);
    intervals += L.nint, need += L.total;
    singles += L.nint == 1;
    max_mcus = L.mcus > max_mcus ? L.mcus : max_mcus;
    max_pixels = (int64_t)it.h * it.w > max_pixels ? (int64_t)it.h * it.w : max_pixels;
    if (need >= (int64_t)k2GiB) return vsp::fail(VSP_ENOTSUP, "jpeg_decode: the work buffer would reach 2 GiB at item %d", i);
  }
  VSP_REQUIRE((uint64_t)need <= work_bytes, "jpeg_decode: work of %zu bytes, these images need %lld", work_bytes, (long long)need);
  hipStream_t s = vsp::as_stream(stream);
  if (hipMemsetAsync(work, 0, (size_t)need, s) != hipSuccess || hipMemsetAsync(status, 0, (size_t)n * 4, s) != hipSuccess ||
      (rounds && hipMemsetAsync(rounds, 0, (size_t)n * 4, s) != hipSuccess))
    return vsp::fail(VSP_ELAUNCH, "jpeg_decode: hipMemsetAsync failed");
  jpeg_dec_unstuff_kernel<<<n, 256, 0, s>>>(in, items_dev, work, status, sub_bytes);
  int rc = vsp::check_launch("jpeg_dec_unstuff");
  if (rc != VSP_OK) return rc;
  if (singles > 0) {
    jpeg_dec_entropy_kernel<1024, true><<<n, 1024, 0, s>>>(items_dev, n, tables_dev, work, status, rounds, sub_bytes);
    rc = vsp::check_launch("jpeg_dec_entropy (one interval)");
    if (rc != VSP_OK) return rc;
  }
  if (singles < n) {
    jpeg_dec_entropy_kernel<64, false><<<(unsigned)intervals, 64, 0, s>>>(items_dev, n, tables_dev, work, status, rounds, sub_bytes);
    rc = vsp::check_launch("jpeg_dec_entropy (restart intervals)");
    if (rc != VSP_OK) return rc;
  }
  jpeg_dec_dc_kernel<<<(unsigned)intervals, 256, 0, s>>>(items_dev, n, work, sub_bytes);
  rc = vsp::check_launch("jpeg_dec_dc");
  if (rc != VSP_OK) return rc;
  jpeg_dec_idct_kernel<<<dim3((unsigned)max_mcus, (unsigned)n), 64, 0, s>>>(items_dev, tables_dev, work, status, sub_bytes);
  rc = vsp::check_launch("jpeg_dec_idct");
  if (rc != VSP_OK) return rc;
  jpeg_dec_color_kernel<<<dim3((unsigned)((max_pixels + 255) / 256), (unsigned)n), 256, 0, s>>>(out, items_dev, work, sub_bytes);
  return vsp::check_launch("jpeg_dec_color");
}

}  // extern "C"
