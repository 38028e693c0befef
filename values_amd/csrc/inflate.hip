// Batched DEFLATE decoder (RFC 1951 inside gzip RFC 1952 / zlib RFC 1950 / raw) -- the reading half of the device
// results tree (values_amd/nifti.py: load_device; values_amd/gz.py: gunzip).  The host reader (nifti.load) inflates
// one file after another on one core.
//
//   inflate_kernel   persistent grid, one wavefront (= one workgroup of 64 lanes) per stream; the waves pull items from
//                    an atomic counter, and the host orders the items by compressed size, largest first.
//     Huffman decode: every lane runs the same serial decode (inflate_core.h) on the same state, so the decode has no
//       divergence and lane j simply keeps token j of the batch (up to 64 tokens); the tables are read from LDS.
//     Tokens go to a 4 KiB staging buffer in LDS: literals lane-parallel, then each match copied by the whole wave in
//       token order (overlapping matches, distance < length: out[o + k] = out[o - d + k mod d]), a wave barrier between
//       matches orders the LDS reads after the writes they depend on.  A source before the staging buffer is read from
//       dst: the staging buffer is flushed to dst (the item's window) with lane-parallel stores followed by
//       __syncthreads(), whose workgroup release / acquire waits for the stores before any later read of them.
//     Input: a 2 KiB window of the compressed bytes in LDS, refilled by the wave (clamped loads) when the reader is
//       less than 1 KiB from its end; a read outside the window falls back to clamped global loads (stream_items.h,
//       which also has the item loop and the launcher's window checks, shared with tiff_lzw.hip).
//     Stored blocks: a lane-parallel copy from the source to dst.
//     Checks: after each member, a second pass over its decoded bytes: the CRC-32 (lane slices joined with
//       crc_join_block) or the Adler-32 (lane slices joined with adler_combine), checksum.h.
// LDS per wave: tables 3.6 KiB + window 2 KiB + staging 4 KiB + checksum joins 0.5 KiB (about 10 KiB): 16 waves per CU.
//
// Every store in this file is a plain C++ store of a vector register.
#include "checksum.h"
#include "inflate_core.h"
#include "stream_items.h"

namespace {

using namespace vxinf;

constexpr int IF_LANES = 64;
constexpr int IF_STAGE = 4096;   // staged output bytes
constexpr int IF_WIN = 2048;     // input window bytes
constexpr int IF_AHEAD = 1024;   // refill when fewer bytes than this lie ahead of the reader in the window
constexpr int IF_WAVES_PER_CU = 16;

struct InfShared {
  uint32_t win[IF_WIN / 4];
  Tables t;
  uint8_t stage[IF_STAGE];
  uint32_t ck[IF_LANES];
  uint32_t cklen[IF_LANES];
};

using DevSrc = vxsi::WinSrc<IF_WIN>;   // the reader's byte source (stream_items.h)
using vxsi::WinItem;                   // spare: the format

__device__ __forceinline__ void win_ensure(InfShared& S, DevSrc& s, const Bits& b) {
  if (s.stale(b.pos, IF_AHEAD)) vxsi::win_load<IF_WIN, IF_LANES>(S.win, s, b.pos);
}

struct Out {
  uint8_t* dst;     // the item's window
  int64_t cap;
  int64_t sbase;    // output index of stage[0]
  int fill;         // staged bytes
};

// staged bytes to dst; afterwards every lane may read them from dst
__device__ void flush(InfShared& S, Out& o) {
  for (int k = threadIdx.x; k < o.fill; k += IF_LANES) o.dst[o.sbase + k] = S.stage[k];
  __syncthreads();
  o.sbase += o.fill;
  o.fill = 0;
}

// one Huffman block with built tables: 0 at its end-of-block code, else a status
__device__ int huffman_block(InfShared& S, DevSrc& s, Bits& b, Out& o, int64_t mstart) {
  const int lane = threadIdx.x;
  const Huff lit = lit_huff(S.t), dist = dist_huff(S.t);
  for (;;) {
    win_ensure(S, s, b);
    if (o.fill > IF_STAGE - 1024) flush(S, o);
    // decode up to 64 tokens (every lane the same); lane j keeps token j
    int tk = 0, ta = 0, td = 0, tp = 0;
    int ntok = 0, bo = o.fill, st = 0;
    bool eob = false;
    while (ntok < IF_LANES && bo + 258 <= IF_STAGE) {
      bits_fill(b, s);
      const int sym = huff_decode(b, lit);
      if (sym < 0 || sym > 285) { st = bits_truncated(b) ? VX_INFLATE_TRUNCATED : VX_INFLATE_BAD_SYMBOL; break; }
      if (sym == 256) {
        if (bits_truncated(b)) st = VX_INFLATE_TRUNCATED;
        else eob = true;
        break;
      }
      int len = 1, d = 0;
      if (sym > 256) {
        len = len_base(sym) + (int)bits_get(b, s, len_extra(sym));
        bits_fill(b, s);
        const int ds = huff_decode(b, dist);
        if (ds < 0 || ds > 29) { st = bits_truncated(b) ? VX_INFLATE_TRUNCATED : VX_INFLATE_BAD_SYMBOL; break; }
        d = dist_base(ds) + (int)bits_get(b, s, dist_extra(ds));
      }
      if (bits_truncated(b)) { st = VX_INFLATE_TRUNCATED; break; }
      const int64_t at = o.sbase + bo;
      if (d > at - mstart) { st = VX_INFLATE_BAD_DISTANCE; break; }
      if (at + len > o.cap) { st = VX_INFLATE_CAPACITY; break; }
      if (lane == ntok) {
        tk = sym > 256 ? 2 : 1;
        ta = sym > 256 ? len : sym;
        td = d;
        tp = bo;
      }
      bo += len;
      ++ntok;
    }
    // the batch: literals lane-parallel, then the matches in order
    if (tk == 1) S.stage[tp] = (uint8_t)ta;
    __syncthreads();
    uint64_t m = __ballot(tk == 2);
    while (m) {
      const int j = __ffsll((unsigned long long)m) - 1;
      m &= m - 1;
      const int L = __builtin_amdgcn_readlane(ta, j);
      const int D = __builtin_amdgcn_readlane(td, j);
      const int P = __builtin_amdgcn_readlane(tp, j);
      for (int k = lane; k < L; k += IF_LANES) {
        const int sp = P - D + (D >= L ? k : k % D);   // < P: bytes written before this match
        const uint8_t v = sp >= 0 ? S.stage[sp] : o.dst[o.sbase + sp];
        S.stage[P + k] = v;
      }
      __syncthreads();
    }
    o.fill = bo;
    if (st || eob) return st;
  }
}

__device__ uint32_t wave_crc32(InfShared& S, const uint8_t* p, int64_t n) {
  const int lane = threadIdx.x;
  const int64_t per = (n + IF_LANES - 1) / IF_LANES;
  const int64_t a = min64(n, per * lane), e = min64(n, a + per);
  uint32_t c = 0xFFFFFFFFu;
  for (int64_t i = a; i < e; ++i) c = kCrc.byte[(c ^ p[i]) & 0xFF] ^ (c >> 8);
  S.ck[lane] = c ^ 0xFFFFFFFFu;
  S.cklen[lane] = (uint32_t)(e - a);
  crc_join_block<IF_LANES>(S.ck, S.cklen);
  const uint32_t r = S.ck[0];
  __syncthreads();
  return r;
}

__device__ uint32_t wave_adler32(InfShared& S, const uint8_t* p, int64_t n) {
  const int lane = threadIdx.x;
  const int64_t per = (n + IF_LANES - 1) / IF_LANES;
  const int64_t a = min64(n, per * lane), e = min64(n, a + per);
  uint32_t x1 = 1, x2 = 0;
  int run = 0;
  for (int64_t i = a; i < e; ++i) {
    x1 += p[i];
    x2 += x1;
    if (++run == 5552) {   // zlib's NMAX: no overflow before the reduction
      x1 %= ADLER_BASE;
      x2 %= ADLER_BASE;
      run = 0;
    }
  }
  S.ck[lane] = ((x2 % ADLER_BASE) << 16) | (x1 % ADLER_BASE);
  S.cklen[lane] = (uint32_t)(e - a);
  for (int stride = 1; stride < IF_LANES; stride <<= 1) {
    __syncthreads();
    if ((lane % (2 * stride)) == 0 && lane + stride < IF_LANES) {
      S.ck[lane] = adler_combine(S.ck[lane], S.ck[lane + stride], S.cklen[lane + stride]);
      S.cklen[lane] += S.cklen[lane + stride];
    }
  }
  __syncthreads();
  const uint32_t r = S.ck[0];
  __syncthreads();
  return r;
}

// one item; *written: bytes in its window
__device__ int inflate_item(InfShared& S, const WinItem& it, uint8_t* dst, int64_t* written) {
  const int format = it.spare;
  const int lane = threadIdx.x;
  DevSrc s{S.win, 0, {it.src, it.src_n}};
  vxsi::win_load<IF_WIN, IF_LANES>(S.win, s, 0);
  Bits b = bits_init(it.src_n);
  Out o{dst, it.dst_cap, 0, 0};
  int st = 0;
  for (;;) {   // members: each one consumes its header, so the loop ends with the input
    const int64_t mstart = o.sbase + o.fill;
    if (format == VX_INFLATE_GZIP) st = gzip_header(b, s);
    else if (format == VX_INFLATE_ZLIB) st = zlib_header(b, s);
    if (st) break;
    int final = 0;
    do {
      win_ensure(S, s, b);
      final = (int)bits_get(b, s, 1);
      const int type = (int)bits_get(b, s, 2);
      if (bits_truncated(b)) { st = VX_INFLATE_TRUNCATED; break; }
      if (type == 0) {
        int len = 0;
        int64_t data = 0;
        st = stored_header(b, s, &len, &data);
        if (st) break;
        flush(S, o);
        if (o.sbase + len > o.cap) { st = VX_INFLATE_CAPACITY; break; }
        for (int k = lane; k < len; k += IF_LANES) o.dst[o.sbase + k] = it.src[data + k];
        __syncthreads();
        o.sbase += len;
        bits_seek(b, s, data + len);
      } else if (type == 3) {
        st = VX_INFLATE_BAD_BLOCK;
      } else {
        __syncthreads();   // the previous block's tables are no longer read
        if (type == 1) fixed_lens(S.t);
        else st = dynamic_lens(b, s, S.t);
        if (!st) st = prepare_block(S.t);
        if (st) break;
        __syncthreads();
        huff_clear(lit_huff(S.t), lane, IF_LANES);
        huff_clear(dist_huff(S.t), lane, IF_LANES);
        __syncthreads();
        huff_fill(lit_huff(S.t), lane, IF_LANES);
        huff_fill(dist_huff(S.t), lane, IF_LANES);
        __syncthreads();
        st = huffman_block(S, s, b, o, mstart);
      }
    } while (!final && !st);
    flush(S, o);
    if (st) break;
    bits_align(b);
    if (format == VX_INFLATE_RAW) {
      if (bits_bytepos(b) < it.src_n) st = VX_INFLATE_TRAILING;
      break;
    }
    win_ensure(S, s, b);
    if (format == VX_INFLATE_ZLIB) {
      const uint32_t ad = trailer_u32(b, s, true);
      if (bits_truncated(b)) st = VX_INFLATE_TRUNCATED;
      else if (ad != wave_adler32(S, o.dst + mstart, o.sbase - mstart)) st = VX_INFLATE_BAD_CHECK;
      else if (bits_bytepos(b) < it.src_n) st = VX_INFLATE_TRAILING;
      break;
    }
    const uint32_t crc = trailer_u32(b, s, false);
    const uint32_t isz = trailer_u32(b, s, false);
    if (bits_truncated(b)) { st = VX_INFLATE_TRUNCATED; break; }
    if (crc != wave_crc32(S, o.dst + mstart, o.sbase - mstart)) { st = VX_INFLATE_BAD_CHECK; break; }
    if (isz != (uint32_t)(o.sbase - mstart)) { st = VX_INFLATE_BAD_ISIZE; break; }
    const int nx = gzip_next(b, s);
    if (nx == 1) continue;
    st = nx;
    break;
  }
  *written = o.sbase + o.fill;
  return st;
}

__global__ __launch_bounds__(IF_LANES) void inflate_kernel(const WinItem* __restrict__ items, int n_items, int* counter,
                                                           uint8_t* dst, int64_t* __restrict__ out_sizes,
                                                           int32_t* __restrict__ out_status) {
  __shared__ InfShared S;
  vxsi::for_each_item(items, n_items, counter, [&](const WinItem& it) {
    int64_t written = 0;
    const int st = inflate_item(S, it, dst + it.dst_off, &written);
    if (threadIdx.x == 0) {
      out_sizes[it.index] = written;
      out_status[it.index] = st;
    }
  });
}

}  // namespace

extern "C" int64_t vx_inflate_workspace_bytes(int n_items) { return vxsi::item_table_bytes(sizeof(WinItem), n_items); }

extern "C" int vx_inflate(const vx_inflate_item* items, int n_items, uint8_t* dst, int64_t dst_n, int64_t* out_sizes,
                          int32_t* out_status, void* workspace, int64_t ws_bytes, vx_stream_t stream) {
  if (n_items < 0) VX_FAIL(VX_E_SHAPE, "vx_inflate: n_items=%d", n_items);
  if (n_items == 0) return VX_OK;
  if (!items || !dst || !out_sizes || !out_status || !workspace) VX_FAIL(VX_E_NULL, "vx_inflate: null pointer");
  const int64_t need = vx_inflate_workspace_bytes(n_items);
  if (ws_bytes < need) VX_FAIL(VX_E_WORKSPACE, "vx_inflate: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)need);
  std::vector<WinItem> di;
  if (int rc = vxsi::win_items("vx_inflate", items, n_items, dst_n, di, [](int i, const vx_inflate_item& g, int32_t* spare) -> int {
        if (g.format < VX_INFLATE_GZIP || g.format > VX_INFLATE_RAW) VX_FAIL(VX_E_DTYPE, "vx_inflate: item %d: format %d", i, g.format);
        *spare = g.format;
        return VX_OK;
      }))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  int grid = 0;
  if (int rc = vxsi::item_table_upload("vx_inflate", workspace, di, s, n_items, IF_WAVES_PER_CU, &grid)) return rc;
  hipLaunchKernelGGL(inflate_kernel, dim3((unsigned)grid), dim3(IF_LANES), 0, s, vxsi::item_table<WinItem>(workspace), n_items,
                     vxsi::item_counter(workspace), dst, out_sizes, out_status);
  VX_CHECK_LAUNCH("vx_inflate");
  return VX_OK;
}
