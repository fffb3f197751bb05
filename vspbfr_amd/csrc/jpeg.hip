// Device-side baseline JPEG encoder for gfx950: the entropy-coded segments of a ragged batch of packed RGB images (format and rules in
// include/vspbfr_hip.h; the host restatement every byte is held to: tests/jpeg_ref.py; the host frames the file, vspbfr_amd/jpeg.py).
//
// A restart interval is an independent, byte-aligned piece of the scan, so the scan is parallel over intervals:
//
//   jpeg_interval_kernel   one wave per interval, MCU after MCU.  Per MCU: pixels -> YCbCr (+ h2v2 downsampling) -> ISLOW DCT in LDS
//                          (jpeg_common.h), then per block lane t owns zig-zag position t: quantise, one ballot gives every non-zero lane
//                          its zero run, the lane builds its whole symbol (up to three ZRL, the run/category code, the value bits: at
//                          most 59 bits in a 64-bit register), a wave scan of the lengths gives its bit offset, and the symbols go to LDS
//                          compacted by the ballot's prefix count.  The bits are then GATHERED: lane t owns output word 64 r + t, finds the
//                          first symbol that reaches into it by binary search over the cumulative lengths and ORs the symbols that
//                          overlap it -- no two lanes share a word, so no atomics.  A second wave scan over the words' byte counts (4 +
//                          their FF bytes) places the stuffed bytes in the interval's slot.  Bits that do not fill a word are carried into
//                          the next MCU as symbol 0; the last MCU appends the 1-bit padding as a symbol.
//   jpeg_scan_kernel       one workgroup per image: exclusive scan of its intervals' byte counts (+ 2 per RSTm marker) and the total
//   jpeg_gather_kernel     one wave per interval: slot -> its place in the image's contiguous segment, RSTm behind it
//
// One wave per interval (not a workgroup of several): every step between two MCUs is a wave-wide ballot or scan, which costs a handful
// of cross-lane instructions and no barrier traffic, and the DC predictors and the carried bits make the MCUs of an interval a serial
// chain anyway; the parallelism comes from the thousands of intervals of a photo.
//
// Bounds: every table entry is checked on the host before the launches (sizes, offsets, interval numbering, slot and segment bounds);
// the byte writer clamps to the slot as well, so not even a wrong bound could make it write outside its slot.
#include "vsp_common.h"
#include "jpeg_common.h"

namespace {

using namespace vsp_jpeg;

constexpr int kMaxSyms = 6 * 64 + 2;   // symbols of one MCU + the carried bits + the padding

// T.81 Annex K.3 Huffman tables as (length << 16 | code), built at compile time from BITS / HUFFVAL
struct HuffSpec {
  unsigned char bits[16];
  unsigned char vals[162];
  int n;
};
constexpr HuffSpec kDcLuma = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr HuffSpec kDcChroma = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr HuffSpec kAcLuma = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    162};
constexpr HuffSpec kAcChroma = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    162};

struct HuffTables {
  uint32_t dc[2][16];    // [luma / chroma][category]
  uint32_t ac[2][256];   // [luma / chroma][run << 4 | category]
};

constexpr void fill_codes(uint32_t* dst, const HuffSpec& s) {
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < s.bits[len - 1]; ++i) dst[s.vals[k++]] = (uint32_t)len << 16 | code++;
    code <<= 1;
  }
}

constexpr HuffTables make_tables() {
  HuffTables t = {};
  fill_codes(t.dc[0], kDcLuma);
  fill_codes(t.dc[1], kDcChroma);
  fill_codes(t.ac[0], kAcLuma);
  fill_codes(t.ac[1], kAcChroma);
  return t;
}

__constant__ HuffTables kHuff = make_tables();

__constant__ unsigned char kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                          41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                          30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Geom {
  int mw, mh, mcus, intervals;
};

__host__ __device__ inline Geom geom(int h, int w, int restart, int sub) {
  const int m = sub == VSP_JPEG_420 ? 16 : 8;
  Geom g;
  g.mw = (w + m - 1) / m, g.mh = (h + m - 1) / m;
  g.mcus = g.mw * g.mh;
  g.intervals = (g.mcus + restart - 1) / restart;
  return g;
}

// the item that owns global interval j: interval0 ascends strictly (checked on the host)
__device__ inline int find_item(const vsp_jpeg_item* items, int n, int j) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (items[mid].interval0 <= j) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ int wave_scan_incl(int v, int t) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d);
    if (t >= d) v += o;
  }
  return v;
}

__device__ __forceinline__ int bit_length(int a) { return 32 - __clz(a); }   // a >= 0; 0 -> 0

// word `wi` (32 bits, MSB first) of the MCU's bit string: symbols s with cumulative end offsets sym_end[s], right-aligned in sym_bits[s]
__device__ inline uint32_t gather_word(const uint64_t* sym_bits, const uint32_t* sym_end, int nsym, int wi) {
  const uint32_t lo = (uint32_t)wi * 32u, hi = lo + 32u;
  int a = 0, b = nsym;                       // first s with sym_end[s] > lo
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (sym_end[mid] > lo) b = mid;
    else a = mid + 1;
  }
  uint32_t word = 0;
  for (int s = a; s < nsym; ++s) {
    const uint32_t end = sym_end[s], start = s ? sym_end[s - 1] : 0u;
    if (start >= hi) break;
    const uint64_t bits = sym_bits[s];
    word |= end <= hi ? (uint32_t)(bits << (hi - end)) : (uint32_t)(bits >> (end - hi));
  }
  return word;
}

// grid (intervals of the call), 64 threads = one wave.  kSub: VSP_JPEG_420 (6 blocks per MCU) or VSP_JPEG_444 (3)
template <int kSub>
__global__ __launch_bounds__(64) void jpeg_interval_kernel(uint8_t* __restrict__ work, int64_t slot, int32_t* __restrict__ counts,
                                                            const uint8_t* __restrict__ src, const vsp_jpeg_item* __restrict__ items, int n,
                                                            int quality, int restart) {
  constexpr int kNb = kSub == VSP_JPEG_420 ? 6 : 3;
  __shared__ int blk[kNb][64];
  __shared__ int qt[2][64];
  __shared__ uint32_t hdc[2][16], hac[2][256];
  __shared__ uint64_t sym_bits[kMaxSyms];
  __shared__ uint32_t sym_end[kMaxSyms];
  const int j = blockIdx.x, t = threadIdx.x;
  const vsp_jpeg_item it = items[find_item(items, n, j)];
  const Geom g = geom(it.h, it.w, restart, kSub);
  const int li = j - it.interval0;
  if (li < 0 || li >= g.intervals) return;
  const int m0 = li * restart, m1 = min(m0 + restart, g.mcus);
  const JpegGeom jg = jpeg_geom(it.h, it.w);
  const int wb = (it.w + 7) >> 3, hb = (it.h + 7) >> 3;
  const uint8_t* img = src + it.src_off;
  auto rgb = [&](int y, int x, int& R, int& G, int& B) {
    const uint8_t* p = img + ((int64_t)y * it.w + x) * 3;
    R = p[0], G = p[1], B = p[2];
  };
  qt[0][t] = jpeg_quant(quality, 0, t);
  qt[1][t] = jpeg_quant(quality, 1, t);
  if (t < 16) hdc[0][t] = kHuff.dc[0][t], hdc[1][t] = kHuff.dc[1][t];
  for (int i = t; i < 256; i += 64) hac[0][i] = kHuff.ac[0][i], hac[1][i] = kHuff.ac[1][i];
  const int zz = kZigzag[t];
  const uint64_t below = (1ull << t) - 1ull;
  uint8_t* out = work + (int64_t)j * slot;
  int pred[3] = {0, 0, 0};       // DC predictors (lane 0's are the ones used)
  uint32_t carry = 0;            // bits of the stream that did not fill a word yet, right-aligned
  int ncarry = 0;
  int opos = 0;                  // bytes written to the slot
  __syncthreads();
  for (int m = m0; m < m1; ++m) {
    const int my = m / g.mw, mx = m - my * g.mw;
    if (kSub == VSP_JPEG_420) {
      const int yy = t >> 2;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int xx = (t & 3) * 4 + q;
        blk[(yy >> 3) * 2 + (xx >> 3)][(yy & 7) * 8 + (xx & 7)] = jpeg_luma(jg, my * 16 + yy, mx * 16 + xx, rgb) - 128;
      }
      int cb, cr;
      jpeg_chroma_h2v2(jg, my * 8 + (t >> 3), mx * 8 + (t & 7), rgb, cb, cr);
      blk[4][t] = cb - 128;
      blk[5][t] = cr - 128;
    } else {
      int R, G, B;
      rgb(min(my * 8 + (t >> 3), it.h - 1), min(mx * 8 + (t & 7), it.w - 1), R, G, B);
      blk[0][t] = rgb_y(R, G, B) - 128;
      blk[1][t] = rgb_cb(R, G, B) - 128;
      blk[2][t] = rgb_cr(R, G, B) - 128;
    }
    __syncthreads();
    if (t < kNb * 8) fdct8<false>(&blk[t >> 3][(t & 7) * 8], 1);
    __syncthreads();
    if (t < kNb * 8) fdct8<true>(&blk[t >> 3][t & 7], 8);
    __syncthreads();
    if (t == 0) sym_bits[0] = carry, sym_end[0] = (uint32_t)ncarry;
    int nsym = 1, bitpos = ncarry;
    int dcs[kNb];                // quantised DC of the MCU's blocks so far (for the dummy blocks)
#pragma unroll
    for (int b = 0; b < kNb; ++b) {
      constexpr int kLuma = kSub == VSP_JPEG_420 ? 4 : 1;
      const int comp = b < kLuma ? 0 : b - kLuma + 1, tbl = comp ? 1 : 0;
      int z = jpeg_quantise(blk[b][zz], qt[tbl][zz]);
      if (kSub == VSP_JPEG_420 && b > 0 && b < 4) {   // a dummy block: AC zero, DC of the block before it / of the row above's last
        const bool row_real = my * 2 + (b >> 1) < hb, real = row_real && mx * 2 + (b & 1) < wb;
        const int prev_dc = (b >= 2 && !row_real) ? dcs[1] : dcs[b > 0 ? b - 1 : 0];
        if (!real) z = t == 0 ? prev_dc : 0;
      }
      dcs[b] = __shfl(z, 0);
      uint64_t bits = 0;
      int len = 0;
      const unsigned long long mask = __ballot(z != 0 && t > 0);
      if (t == 0) {
        const int diff = z - pred[comp];
        const int cat = bit_length(diff < 0 ? -diff : diff);
        const uint32_t e = hdc[tbl][cat];
        bits = ((uint64_t)(e & 0xFFFFu) << cat) | (uint32_t)((diff < 0 ? diff - 1 : diff) & ((1 << cat) - 1));
        len = (int)(e >> 16) + cat;
      } else if (z != 0) {
        const unsigned long long pm = mask & below;
        const int prev = pm ? 63 - __clzll((long long)pm) : 0;
        const int run = t - prev - 1;
        const int cat = bit_length(z < 0 ? -z : z);
        const uint32_t zrl = hac[tbl][0xF0], e = hac[tbl][((run & 15) << 4) | cat];
        for (int i = 0; i < (run >> 4); ++i) bits = (bits << (zrl >> 16)) | (zrl & 0xFFFFu);
        bits = (bits << (e >> 16)) | (e & 0xFFFFu);
        bits = (bits << cat) | (uint32_t)((z < 0 ? z - 1 : z) & ((1 << cat) - 1));
        len = (run >> 4) * (int)(zrl >> 16) + (int)(e >> 16) + cat;
      } else if (t == 63) {      // the block ends in zeros: EOB
        const uint32_t e = hac[tbl][0];
        bits = e & 0xFFFFu;
        len = (int)(e >> 16);
      }
      pred[comp] = z;            // lane 0: the DC
      const unsigned long long emask = __ballot(len > 0);
      const int incl = wave_scan_incl(len, t);
      if (len > 0) {
        const int idx = nsym + __popcll(emask & below);
        sym_bits[idx] = bits;
        sym_end[idx] = (uint32_t)(bitpos + incl);
      }
      nsym += __popcll(emask);
      bitpos += __shfl(incl, 63);
    }
    const bool last = m == m1 - 1;
    if (last && (bitpos & 7)) {  // pad the interval's last byte with 1-bits
      const int pad = 8 - (bitpos & 7);
      if (t == 0) sym_bits[nsym] = (1u << pad) - 1u, sym_end[nsym] = (uint32_t)(bitpos + pad);
      nsym += 1;
      bitpos += pad;
    }
    __syncthreads();
    // whole words, and at the interval's end the bytes of the last partial word
    const int nwords = last ? (bitpos + 31) >> 5 : bitpos >> 5;
    const int nbytes = last ? bitpos >> 3 : (bitpos >> 5) * 4;
    for (int w0 = 0; w0 < nwords; w0 += 64) {
      const int wi = w0 + t;
      uint32_t word = 0;
      int nb = 0, olen = 0;
      if (wi < nwords) {
        word = gather_word(sym_bits, sym_end, nsym, wi);
        nb = min(4, nbytes - wi * 4);
        for (int k = 0; k < nb; ++k) olen += 1 + (((word >> (24 - 8 * k)) & 255u) == 255u);
      }
      const int incl = wave_scan_incl(olen, t);
      int o = opos + incl - olen;
      for (int k = 0; k < nb; ++k) {
        const uint32_t byte = (word >> (24 - 8 * k)) & 255u;
        if (o < slot) out[o] = (uint8_t)byte;
        ++o;
        if (byte == 255u) {
          if (o < slot) out[o] = 0;
          ++o;
        }
      }
      opos += __shfl(incl, 63);
    }
    if (!last) {
      ncarry = bitpos & 31;
      carry = ncarry ? gather_word(sym_bits, sym_end, nsym, bitpos >> 5) >> (32 - ncarry) : 0u;
    }
    __syncthreads();             // the symbol list and the blocks are rewritten by the next MCU
  }
  if (t == 0) counts[j] = opos;
}

// grid (n), 256 threads: offs[interval] = bytes of the image's segment in front of it, totals[i] = bytes of the segment
__global__ __launch_bounds__(256) void jpeg_scan_kernel(int32_t* __restrict__ offs, int32_t* __restrict__ totals,
                                                        const int32_t* __restrict__ counts, const vsp_jpeg_item* __restrict__ items,
                                                        int64_t slot, int sub, int restart) {
  __shared__ int part[256];
  const vsp_jpeg_item it = items[blockIdx.x];
  const int nint = geom(it.h, it.w, restart, sub).intervals, t = threadIdx.x;
  int running = 0;
  for (int base = 0; base < nint; base += 256) {
    const int idx = base + t;
    const int v = idx < nint ? min(max(counts[it.interval0 + idx], 0), (int)slot) + (idx < nint - 1 ? 2 : 0) : 0;
    part[t] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const int o = t >= d ? part[t - d] : 0;
      __syncthreads();
      part[t] += o;
      __syncthreads();
    }
    if (idx < nint) offs[it.interval0 + idx] = running + part[t] - v;
    running += part[255];
    __syncthreads();
  }
  if (t == 0) totals[blockIdx.x] = running;
}

// grid (intervals of the call), 64 threads: the interval's bytes to their place, then FF D0 + (k mod 8) unless it is the image's last
__global__ __launch_bounds__(64) void jpeg_gather_kernel(uint8_t* __restrict__ out, int64_t out_bytes, const uint8_t* __restrict__ work, int64_t slot,
                                                         const int32_t* __restrict__ counts, const int32_t* __restrict__ offs,
                                                         const vsp_jpeg_item* __restrict__ items, int n, int sub, int restart) {
  const int j = blockIdx.x, t = threadIdx.x;
  const vsp_jpeg_item it = items[find_item(items, n, j)];
  const int nint = geom(it.h, it.w, restart, sub).intervals, li = j - it.interval0;
  if (li < 0 || li >= nint) return;
  const int nb = min(max(counts[j], 0), (int)slot);
  const uint8_t* s = work + (int64_t)j * slot;
  if (offs[j] < 0 || it.out_off + offs[j] + nb + 2 > out_bytes) return;   // cannot happen with counts inside their bounds
  uint8_t* d = out + it.out_off + offs[j];
  for (int i = t; i < nb; i += 64) d[i] = s[i];
  if (li < nint - 1 && t < 2) d[nb + t] = t ? (uint8_t)(0xD0 + (li & 7)) : (uint8_t)0xFF;
}

bool sub_ok(int sub) { return sub == VSP_JPEG_444 || sub == VSP_JPEG_420; }

constexpr size_t k2GiB = (size_t)1 << 31;

}  // namespace

extern "C" {

int vsp_jpeg_intervals(int h, int w, int restart, int subsampling) {
  if (h < 1 || h > 65535 || w < 1 || w > 65535 || restart < 1 || restart > 65535 || !sub_ok(subsampling)) return 0;
  return geom(h, w, restart, subsampling).intervals;
}

size_t vsp_jpeg_interval_bound(int mcus, int subsampling) {
  if (mcus < 1 || !sub_ok(subsampling)) return 0;
  return (size_t)mcus * (subsampling == VSP_JPEG_420 ? 6 : 3) * VSP_JPEG_BLOCK_BOUND + 4;
}

size_t vsp_jpeg_image_bound(int h, int w, int restart, int subsampling) {
  if (vsp_jpeg_intervals(h, w, restart, subsampling) == 0) return 0;
  const Geom g = geom(h, w, restart, subsampling);
  return (size_t)g.mcus * (subsampling == VSP_JPEG_420 ? 6 : 3) * VSP_JPEG_BLOCK_BOUND + (size_t)g.intervals * 6;
}

int vsp_jpeg_encode_u8(uint8_t* out, size_t out_bytes, int32_t* totals, uint8_t* work, size_t work_bytes, int32_t* interval_ws,
                       const uint8_t* src, size_t src_bytes, const vsp_jpeg_item* items, const vsp_jpeg_item* items_dev, int n,
                       int quality, int subsampling, int restart, vsp_stream_t stream) {
  VSP_REQUIRE(n >= 0 && n <= VSP_JPEG_MAX_ITEMS, "jpeg_encode: %d items (max %d)", n, VSP_JPEG_MAX_ITEMS);
  VSP_REQUIRE(quality >= 1 && quality <= 100, "jpeg_encode: quality %d outside 1..100", quality);
  VSP_REQUIRE(sub_ok(subsampling), "jpeg_encode: subsampling %d (VSP_JPEG_444 or VSP_JPEG_420)", subsampling);
  VSP_REQUIRE(restart >= 1 && restart <= 65535, "jpeg_encode: restart interval %d outside 1..65535", restart);
  if (n == 0) return VSP_OK;
  VSP_REQUIRE(out && totals && work && interval_ws && src && items && items_dev, "jpeg_encode: null pointer");
  if (src_bytes >= k2GiB || out_bytes >= k2GiB || work_bytes >= k2GiB)
    return vsp::fail(VSP_ENOTSUP, "jpeg_encode: a buffer of 2 GiB or more (src %zu, out %zu, work %zu)", src_bytes, out_bytes, work_bytes);
  int64_t total = 0;
  int max_mcus = 0;
  for (int i = 0; i < n; ++i) {
    const vsp_jpeg_item& it = items[i];
    VSP_REQUIRE(it.h >= 1 && it.h <= 65535 && it.w >= 1 && it.w <= 65535, "jpeg_encode: item %d is %d x %d (1..65535)", i, it.h, it.w);
    VSP_REQUIRE(it.src_off >= 0 && (uint64_t)it.src_off + (uint64_t)it.h * it.w * 3 <= src_bytes, "jpeg_encode: item %d lies outside src", i);
    VSP_REQUIRE(it.out_off >= 0 && (uint64_t)it.out_off + vsp_jpeg_image_bound(it.h, it.w, restart, subsampling) <= out_bytes,
                "jpeg_encode: the segment bound of item %d lies outside out", i);
    VSP_REQUIRE(it.interval0 == total, "jpeg_encode: item %d has interval0 %d, expected %lld", i, it.interval0, (long long)total);
    const Geom g = geom(it.h, it.w, restart, subsampling);
    total += g.intervals;
    max_mcus = g.mcus > max_mcus ? g.mcus : max_mcus;
    if (total >= (int64_t)k2GiB) return vsp::fail(VSP_ENOTSUP, "jpeg_encode: 2^31 restart intervals or more");
  }
  const size_t slot = vsp_jpeg_interval_bound(restart < max_mcus ? restart : max_mcus, subsampling);
  if ((uint64_t)total * slot >= k2GiB)
    return vsp::fail(VSP_ENOTSUP, "jpeg_encode: %lld intervals of %zu bytes need a work buffer of 2 GiB or more", (long long)total, slot);
  VSP_REQUIRE((uint64_t)total * slot <= work_bytes, "jpeg_encode: work of %zu bytes, %lld intervals of %zu bytes need %llu", work_bytes,
              (long long)total, slot, (unsigned long long)((uint64_t)total * slot));
  int32_t* counts = interval_ws;
  int32_t* offs = interval_ws + total;
  hipStream_t s = vsp::as_stream(stream);
  if (subsampling == VSP_JPEG_420)
    jpeg_interval_kernel<VSP_JPEG_420><<<(unsigned)total, 64, 0, s>>>(work, (int64_t)slot, counts, src, items_dev, n, quality, restart);
  else
    jpeg_interval_kernel<VSP_JPEG_444><<<(unsigned)total, 64, 0, s>>>(work, (int64_t)slot, counts, src, items_dev, n, quality, restart);
  int rc = vsp::check_launch("jpeg_interval");
  if (rc != VSP_OK) return rc;
  jpeg_scan_kernel<<<n, 256, 0, s>>>(offs, totals, counts, items_dev, (int64_t)slot, subsampling, restart);
  rc = vsp::check_launch("jpeg_scan");
  if (rc != VSP_OK) return rc;
  jpeg_gather_kernel<<<(unsigned)total, 64, 0, s>>>(out, (int64_t)out_bytes, work, (int64_t)slot, counts, offs, items_dev, n,
                                                       subsampling, restart);
  return vsp::check_launch("jpeg_gather");
}

}  // extern "C"
