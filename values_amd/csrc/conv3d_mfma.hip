// K1: 3x3x3 convolution (padding 1), channels-last fp32, as an implicit GEMM on the gfx950
// fp32 matrix cores (v_mfma_f32_16x16x4_f32: exact fp32 FMA chain, same numerics as VALU).
//
//   GEMM view:  D[row][col] = sum_k  A[row][k] * B[k][col]
//   A operand = weights  (lane l holds A[row = l&15][k = l>>4])
//   B operand = inputs   (lane l holds B[k = l>>4][col = l&15])
//   D: lane l holds rows (l>>4)*4 + {0..3} of column l&15 -> 4 consecutive output channels of one voxel,
//      so the epilogue is ONE 16-byte store per lane and a wave writes 1 KiB contiguously.
//
// Two packings of the 16x16 tile:
//   plain (XP = 0): rows = 16 output channels, cols = 16 voxels of an x-row, k = (kz,ky,kx, cin): 27*Cin.
//   x-pair (XP = 1, Cout == 8): a 16-wide tile would be half padding, so two x-adjacent outputs share it:
//      rows = (dx in {0,1}, cout 0..7), cols = 16 voxel PAIRS (x = 2p, 2p+1), k = (kz,ky, ix in 0..3, cin) where
//      input x = 2p + ix - 1 and the weight is W[kx = ix - dx] (zero when ix - dx is outside 0..2).
//      K grows by 4/3 while the columns cover twice the voxels: 1.5x fewer MFMAs (75 % dense instead of 50 %).
//
// Work split: a workgroup of NW waves owns an output tile of TXV x TY x TZ voxels (TXV = 16, or 32 for x-pair)
// for 16*NT rows; each wave owns R column tiles and all NT row tiles: R*NT independent accumulators.
// Cin is consumed in chunks of CB (8 or 16) channels: per chunk the halo'd input tile [HZ][HY][HX][CB] and the
// chunk's weights [taps][NT][64 lanes][CB/4] sit in LDS; a lane's CB/4 consecutive channels come from one
// ds_read_b128 (b64 for CB = 8) and feed CB/4 MFMAs.
//
// Schedule: persistent workgroups walk a flat list of (tile, chunk) work items.  While item i computes, the global
// loads of item i+1 are already in flight into registers (buffer loads: out-of-volume halo pieces are steered
// out of the descriptor's range and come back as zeros -- no branches, ~3 VALU per 16-byte piece); they are
// committed to LDS after the barrier that ends item i.  Single-chunk layers keep their weights resident in LDS.
// Non-MFMA instructions are the enemy here (they compete with the matrix pipe for the SIMD's issue port), so
// everything per-lane that does not change between tiles is computed once per workgroup.
//
// Input layouts: plain [N][D][H][W][pitch], or the decoder's x-blocked concat buffer
// [N][D][H][W/xb][2][xb][C] (up half, skip half as alternating dense blocks; see unet3d_forward.hip).
//
// Epilogue (fused): bias, then either (a) raw store + per-workgroup (sum, sumsq) partials for the
// InstanceNorm that follows (contract blocks), or (b) LeakyReLU/ReLU + dropout (expand / center).
#include "conv3d_internal.h"

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct ConvKArgs {
  vx_conv3d_args a;
  int tiles_x, tiles_y, tiles_z, nchunks;
  unsigned mx, my, mz;  // floor(2^32 / tiles_*) + 1: exact t / tiles_* = umulhi(t, m) for t * tiles_* < 2^32
  unsigned long long* dbg;  // VX_CONV_STAMPS diagnostic builds only
};

constexpr unsigned VX_OOB = 0xFFFFFFF0u;      // voffset beyond every descriptor's num_records
constexpr unsigned VX_NUMREC = 0x80000000u;

template <int CB, int NT, int TX, int TY, int TZ, int NW, int XP>
__global__ __launch_bounds__(64 * NW) void conv3d_k3_mfma_kernel(ConvKArgs ka) {
  constexpr int NTH = 64 * NW;                     // threads per workgroup
  constexpr int CPL = CB / 4;                      // channels per lane per tap
  constexpr int TXV = XP ? 2 * TX : TX;            // voxels per tile along x (TX = columns per column tile = 16)
  constexpr int NVT = TX * TY * TZ / 16;           // column tiles per workgroup
  constexpr int R = NVT / NW;                      // column tiles per wave
  constexpr int HX = TXV + 2, HY = TY + 2, HZ = TZ + 2;
  constexpr int NHALO = HX * HY * HZ;
  // LDS image of the input tile: [g = channel group of CPL][parity plane (x-pair only)][position][CPL floats].
  // A lane (column m, k-group g) reads CPL floats at position p0 + m of plane g: the 16 columns of a tile are
  // CONSECUTIVE positions, so a wave's read is conflict-free whatever the tap offset (plane size: see PLANE),
  // and every tap is an immediate offset.  x-pair columns are 2 voxels apart, so even and odd x live in
  // separate parity planes and stay consecutive.
  constexpr int NPAR = XP ? 2 : 1;
  constexpr int HXP = XP ? HX / 2 : HX;            // positions per x-row (per parity)
  constexpr int NPP = HXP * HY * HZ;               // positions per parity plane
  // positions per g-plane, padded so that plane stride keeps the 4 k-groups on disjoint banks:
  // 16-byte reads (CB=16): multiple of 16 positions; 8-byte reads (CB=8): 16 mod 32 positions
  constexpr int PLANE = CB == 16 ? ((NPAR * NPP + 15) / 16) * 16 : ((NPAR * NPP + 15) / 32) * 32 + 16;
  constexpr int IN_FLOATS = 4 * PLANE * (CB / 4);
  constexpr int NTAP = XP ? 36 : 27;
  constexpr int W_FLOATS = NTAP * NT * 64 * CPL;
  constexpr int Q = CB / 4;                        // 16-byte pieces per voxel
  constexpr int IN_IT = (NHALO * Q + NTH - 1) / NTH;   // staging iterations per thread (input tile)
  constexpr int W_IT = (W_FLOATS / 4 + NTH - 1) / NTH; // staging iterations per thread (weights)
  static_assert(NVT % NW == 0, "tile must give each wave a whole number of column tiles");
  static_assert(IN_IT <= 16, "invalid-piece masks are 16 bits per class");
  static_assert(!XP || NT == 1, "x-pair packing is for Cout == 8");
  typedef float vecc __attribute__((ext_vector_type(CPL)));

  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* s_in = smem;
  float* s_w = smem + IN_FLOATS;

  const vx_conv3d_args& a = ka.a;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int m = lane & 15;   // column within column tile (B) / row within row tile (A)
  const int g = lane >> 4;   // k index within the MFMA's K=4; D rows 4g..4g+3
  const int cg = blockIdx.y;  // row group of 16*NT (plain) -- always 0 for x-pair
  const int ntiles = ka.tiles_x * ka.tiles_y * ka.tiles_z;
  const int total = ntiles * a.N;
  const int lastx = (ka.tiles_x - 1) * TXV, lasty = (ka.tiles_y - 1) * TY, lastz = (ka.tiles_z - 1) * TZ;

  // ---- per-lane constants of the compute phase and of the epilogue (identical for every tile) ----
  int vbase[R];      // LDS float index of the lane's B fragment at tap (0,0,0)
  unsigned ovoff[R]; // byte offset of the lane's output piece relative to the tile origin (rows of row tile 0)
  unsigned eoff[R];  // element index (dropout / mask) of the same, relative to the tile origin
  unsigned obad_xhi = 0, obad_yhi = 0, obad_zhi = 0;  // bit r: piece outside the volume in the last tile of that axis
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int v = (wave * R + r) * 16 + m;                 // column index within the workgroup tile
    const int cx = v % TX, ly = (v / TX) % TY, lz = v / (TX * TY);
    const int lx = XP ? 2 * cx : cx;                       // first voxel of the column
    vbase[r] = (g * PLANE + (lz * HY + ly) * HXP + cx) * CPL;
    const int ox = XP ? lx + (g >> 1) : lx;                // voxel this lane stores
    const int oc = XP ? (g & 1) * 4 : g * 4;               // its first channel (within row tile 0)
    const int ovox = (lz * a.H + ly) * a.W + ox;
    ovoff[r] = (unsigned)((ovox * a.out_pitch + a.out_coff + oc) * 4);
    eoff[r] = (unsigned)(ovox * a.Cout + oc);
    if (ox >= a.W - lastx) obad_xhi |= 1u << r;
    if (ly >= a.H - lasty) obad_yhi |= 1u << r;
    if (lz >= a.D - lastz) obad_zhi |= 1u << r;
  }

  // ---- per-thread staging pattern (identical for every tile) ----
  // input rows: plain: voxel stride in_pitch; x-blocked concat: [W/xb][2][xb][C], C = Cin/2
  const int xb = a.in_xblk;
  const int Csrc = xb ? a.Cin / 2 : a.Cin;
  const int voxf = xb ? 2 * Csrc : a.in_pitch;           // floats per voxel step along x (row average)
  const int rowf = a.W * voxf;                           // floats per x-row
  const int biasf = (a.H + 1) * rowf + 4 * voxf;          // keeps every voffset non-negative
  unsigned voff[IN_IT];
  int ldst[IN_IT];   // LDS float index of the piece's first channel group (a 16-byte piece spans 4/CPL groups)
  unsigned ibad_always = 0, ibad_xlo = 0, ibad_xhi = 0, ibad_ylo = 0, ibad_yhi = 0, ibad_zlo = 0, ibad_zhi = 0;
#pragma unroll
  for (int it = 0; it < IN_IT; ++it) {
    const int idx = tid + it * NTH;
    const int vox = idx / Q, q = idx % Q;
    const int hx = vox % HX, hy = (vox / HX) % HY, hz = vox / (HX * HY);
    const int dxr = hx - 1, dyr = hy - 1, dzr = hz - 1;   // voxel relative to the tile origin
    int xf;                                               // float offset of (dxr, channel 4q) within its row
    if (xb) {
      const int blk = dxr >= 0 ? dxr / xb : -((-dxr + xb - 1) / xb);
      const int rem = dxr - blk * xb;
      const int sl = (Csrc < CB) ? (4 * q) / Csrc : 0;    // C < CB: the chunk spans both halves
      const int cs = (Csrc < CB) ? (4 * q) % Csrc : 4 * q;
      xf = (blk * 2 + sl) * xb * Csrc + rem * Csrc + cs;
    } else {
      xf = dxr * a.in_pitch + 4 * q;
    }
    const int rel = (dzr * a.H + dyr) * rowf + xf;
    voff[it] = (unsigned)((rel + biasf) * 4);
    {
      const int par = XP ? (hx & 1) : 0, px = XP ? (hx >> 1) : hx;
      const int pos = par * NPP + (hz * HY + hy) * HXP + px;
      ldst[it] = ((q * (4 / CPL)) * PLANE + pos) * CPL;
    }
    if (idx >= NHALO * Q) ibad_always |= 1u << it;
    if (dxr < 0) ibad_xlo |= 1u << it;
    if (dxr >= a.W - lastx) ibad_xhi |= 1u << it;
    if (dyr < 0) ibad_ylo |= 1u << it;
    if (dyr >= a.H - lasty) ibad_yhi |= 1u << it;
    if (dzr < 0) ibad_zlo |= 1u << it;
    if (dzr >= a.D - lastz) ibad_zhi |= 1u << it;
  }
  const size_t in_sample = (size_t)a.D * a.H * rowf;
  const size_t out_sample = (size_t)a.D * a.H * a.W * a.out_pitch;
  const int cper = xb && Csrc >= CB ? Csrc / CB : 0;      // chunks per concat half (0: not chunk-uniform)

  auto decode = [&](int tile_lin, int& n, int& tx, int& ty, int& tz) {
    unsigned t = (unsigned)tile_lin, q;
    q = ka.tiles_x == 1 ? t : __umulhi(t, ka.mx); tx = (int)(t - q * ka.tiles_x); t = q;
    q = ka.tiles_y == 1 ? t : __umulhi(t, ka.my); ty = (int)(t - q * ka.tiles_y); t = q;
    q = ka.tiles_z == 1 ? t : __umulhi(t, ka.mz); tz = (int)(t - q * ka.tiles_z); n = (int)q;
  };

  const float* w_cg = a.w_packed + (size_t)cg * ka.nchunks * W_FLOATS;
  f32x4 ibuf[IN_IT];
  f32x4 wbuf[W_IT];
  const bool w_resident = ka.nchunks == 1;  // single-chunk layers: the weights never change, stage them once
  bool w_fresh = true;

  // issue the global loads of one (tile, chunk) work item into registers (no wait)
  auto prefetch = [&](int tile_lin, int chunk, bool have, bool with_w) {
    int n, tx, ty, tz;
    decode(tile_lin, n, tx, ty, tz);
    unsigned bad = ibad_always;
    if (tx == 0) bad |= ibad_xlo;
    if (tx == ka.tiles_x - 1) bad |= ibad_xhi;
    if (ty == 0) bad |= ibad_ylo;
    if (ty == ka.tiles_y - 1) bad |= ibad_yhi;
    if (tz == 0) bad |= ibad_zlo;
    if (tz == ka.tiles_z - 1) bad |= ibad_zhi;
    if (!have) bad = 0xFFFFFFFFu;
    int coff;  // float offset of this chunk's first channel
    if (!xb) coff = chunk * CB;
    else if (cper) coff = (chunk / cper) * xb * Csrc + (chunk % cper) * CB;
    else coff = 0;
    const unsigned soff = (unsigned)((((tz * TZ) * a.H + ty * TY) * rowf + tx * TXV * voxf + coff) * 4);
    const __amdgpu_buffer_rsrc_t srd = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(a.in + (size_t)(have ? n : 0) * in_sample - biasf), 0, VX_NUMREC, 0x00020000);
#pragma unroll
    for (int it = 0; it < IN_IT; ++it) {
      const unsigned vo = ((bad >> it) & 1u) ? VX_OOB : voff[it];
      ibuf[it] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srd, (int)vo, (int)soff, 0));
    }
    const f32x4* src = reinterpret_cast<const f32x4*>(w_cg + (size_t)chunk * W_FLOATS);
#pragma unroll
    for (int it = 0; it < W_IT; ++it) {
      const int idx = tid + it * NTH;
      f32x4 v = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (have && with_w && idx < W_FLOATS / 4) v = src[idx];
      wbuf[it] = v;
    }
  };
  auto commit = [&](bool with_w) {
#pragma unroll
    for (int it = 0; it < IN_IT; ++it) {
      const int idx = tid + it * NTH;
      if (idx < NHALO * Q) {
        if (CPL == 4) {
          *reinterpret_cast<f32x4*>(s_in + ldst[it]) = ibuf[it];
        } else {  // CB = 8: the piece's two channel pairs belong to two g-planes
          *reinterpret_cast<f32x2*>(s_in + ldst[it]) = (f32x2){ibuf[it][0], ibuf[it][1]};
          *reinterpret_cast<f32x2*>(s_in + ldst[it] + PLANE * CPL) = (f32x2){ibuf[it][2], ibuf[it][3]};
        }
      }
    }
    if (with_w) {
#pragma unroll
      for (int it = 0; it < W_IT; ++it) {
        const int idx = tid + it * NTH;
        if (idx < W_FLOATS / 4) reinterpret_cast<f32x4*>(s_w)[idx] = wbuf[it];
      }
    }
  };

  // bias once per workgroup: a load inside the loop would sit behind the prefetch loads in the in-order vmcnt
  // queue and make every epilogue wait for the NEXT tile's data
  f32x4 bias4[NT];
  bool cvalid[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int co = XP ? (g & 1) * 4 : (cg * NT + nt) * 16 + g * 4;
    cvalid[nt] = co < a.Cout;
    bias4[nt] = cvalid[nt] ? *reinterpret_cast<const f32x4*>(a.bias + co) : (f32x4){0.f, 0.f, 0.f, 0.f};
  }

  // One flat loop over (tile, chunk) work items: commit the prefetched registers to LDS, issue the NEXT item's
  // global loads (straight-line, predicated -- no loop-carried register copies that would force a vmcnt(0)),
  // compute this item, and run the epilogue after a tile's last chunk.
  // XCD-aware tile order (see conv3d_c8.hip): each XCD takes a contiguous run of tiles per round
  int tile_lin = blockIdx.x, chunk = 0;
  if ((gridDim.x & 7) == 0) tile_lin = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
  bool have = tile_lin < total;
  prefetch(tile_lin, 0, have, true);
  f32x4 acc[R][NT];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[r][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

#ifdef VX_CONV_STAMPS
  unsigned long long st_sum[6] = {0, 0, 0, 0, 0, 0}, st_last, st_iters = 0;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_last)::"memory");
#endif
  while (have) {
    __syncthreads();   // everyone finished reading the previous item from LDS
    VX_STAMP(0);
    commit(w_fresh);   // (waits for the prefetched loads)
    VX_STAMP(1);
    __syncthreads();
    VX_STAMP(2);
    w_fresh = !w_resident;
    int ntile = tile_lin, nchunk = chunk + 1;
    if (nchunk == ka.nchunks) { nchunk = 0; ntile = tile_lin + (int)gridDim.x; }
    const bool nhave = ntile < total;
    prefetch(ntile, nchunk, nhave, !w_resident);
    VX_STAMP(3);

    {
      // ---- NTAP taps x CPL MFMAs x R x NT; fragments are read PD taps ahead of their MFMAs ----
      constexpr int PD = CB == 8 ? 3 : 1;  // CB = 8 has only 2*R*NT MFMAs per tap to cover an LDS read
      constexpr int NB = PD + 1;
      vecc wf[NB][NT], xf[NB][R];
      auto load_tap = [&](int t1, int slot) {
        // plain: tap = (kz*3 + ky)*3 + kx ; x-pair: tap = (kz*3 + ky)*4 + ix
        const int kz = XP ? t1 / 12 : t1 / 9, ky = XP ? (t1 / 4) % 3 : (t1 / 3) % 3, kx = XP ? t1 % 4 : t1 % 3;
        // x-pair: tap ix reads voxel 2p + ix -> parity ix & 1, position p + (ix >> 1)
        const int toff = (XP ? (kx & 1) * NPP + (kz * HY + ky) * HXP + (kx >> 1) : (kz * HY + ky) * HXP + kx) * CPL;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          wf[slot][nt] = *reinterpret_cast<const vecc*>(s_w + ((t1 * NT + nt) * 64 + lane) * CPL);
#pragma unroll
        for (int r = 0; r < R; ++r) xf[slot][r] = *reinterpret_cast<const vecc*>(s_in + vbase[r] + toff);
      };
#pragma unroll
      for (int t = 0; t < PD; ++t) load_tap(t, t);
#pragma unroll
      for (int tap = 0; tap < NTAP; ++tap) {
        if (tap + PD < NTAP) load_tap(tap + PD, (tap + PD) % NB);
        const int cur = tap % NB;
#pragma unroll
        for (int j = 0; j < CPL; ++j)
#pragma unroll
          for (int r = 0; r < R; ++r)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
              acc[r][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[cur][nt][j], xf[cur][r][j], acc[r][nt], 0, 0, 0);
      }
    }

    VX_STAMP(4);
    if (chunk == ka.nchunks - 1) {
      // ---- epilogue ----
      int n, tx, ty, tz;
      decode(tile_lin, n, tx, ty, tz);
      unsigned obad = 0;
      if (tx == ka.tiles_x - 1) obad |= obad_xhi;
      if (ty == ka.tiles_y - 1) obad |= obad_yhi;
      if (tz == ka.tiles_z - 1) obad |= obad_zhi;
      const unsigned vox0 = (unsigned)(((tz * TZ) * a.H + ty * TY) * a.W + tx * TXV);  // tile origin voxel (in sample)
      const unsigned osoff = vox0 * (unsigned)a.out_pitch * 4u;
      const unsigned e0 = vox0 * (unsigned)a.Cout;
      const __amdgpu_buffer_rsrc_t osrd =
          __builtin_amdgcn_make_buffer_rsrc((void*)(a.out + (size_t)n * out_sample), 0, VX_NUMREC, 0x00020000);
      const vx_dkey dkey = vx_drop_key(vx_seed_of(a, a.drop_seed), a.drop_layer, (uint32_t)n);

      float ssum[NT][4], ssq[NT][4];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int j = 0; j < 4; ++j) { ssum[nt][j] = 0.f; ssq[nt][j] = 0.f; }

#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const unsigned cshift = XP ? 0u : (unsigned)((cg * NT + nt) * 16);  // first channel of this row tile
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const bool bad = ((obad >> r) & 1u) || !cvalid[nt];
          f32x4 v = acc[r][nt] + bias4[nt];
          if (a.stats_partial && !bad) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { ssum[nt][j] += v[j]; ssq[nt][j] += v[j] * v[j]; }
          }
          if (a.act == VX_ACT_LRELU) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.01f * v[j]);
          } else if (a.act == VX_ACT_RELU) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
          }
          const unsigned e = e0 + eoff[r] + cshift;
          if (a.drop_mode == VX_DROP_HASH) {
            const uint32_t bits = vx_drop_bits4(dkey, e);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] *= __uint_as_float((bits << (30 - j)) & 0x40000000u);  // keep ? 2 : 0
          } else if (a.drop_mode == VX_DROP_MASK) {
            uint32_t mk = 0;
            if (!bad) mk = *reinterpret_cast<const uint32_t*>(a.drop_mask + (size_t)n * a.D * a.H * a.W * a.Cout + e);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = ((mk >> (8 * j)) & 0xFFu) ? 2.f * v[j] : 0.f;
          }
          const unsigned vo = bad ? VX_OOB : ovoff[r] + cshift * 4u;
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), osrd, (int)vo, (int)osoff, 0);
          // gfx950: a 16-byte buffer store with an SGPR soffset still reads its data registers for a few cycles
          // after issue; hipcc (ROCm 7.2) pads this hazard only for an immediate soffset, so the next VALU write
          // of those registers corrupted the last beat (dword 3, lanes 12-15 of each row).  Pad it by hand.
          __builtin_amdgcn_sched_barrier(0);
          asm volatile("s_nop 3" ::: "memory");
          __builtin_amdgcn_sched_barrier(0);
        }
      }

      if (a.stats_partial) {
        // reduce over the 16 lanes that share g -> per-wave sums per row, then over waves via LDS
        float* s_red = smem + IN_FLOATS + W_FLOATS;  // [NW waves][NT][16 rows][2], outside the staged tiles
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float s = ssum[nt][j], q = ssq[nt][j];
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) {
              s += __shfl_xor(s, off, 64);
              q += __shfl_xor(q, off, 64);
            }
            if (m == 0) {
              s_red[((wave * NT + nt) * 16 + g * 4 + j) * 2 + 0] = s;
              s_red[((wave * NT + nt) * 16 + g * 4 + j) * 2 + 1] = q;
            }
          }
        __syncthreads();
        if (tid < NT * 16) {
          const int nt = tid / 16, c = tid % 16;
          // x-pair: rows c and c+8 are the two x-parities of channel c
          const int co = XP ? c : (cg * NT + nt) * 16 + c;
          if (co < a.Cout && (!XP || c < 8)) {
            float s = 0.f, q = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
              s += s_red[((w * NT + nt) * 16 + c) * 2 + 0];
              q += s_red[((w * NT + nt) * 16 + c) * 2 + 1];
              if (XP) {
                s += s_red[((w * NT + nt) * 16 + c + 8) * 2 + 0];
                q += s_red[((w * NT + nt) * 16 + c + 8) * 2 + 1];
              }
            }
            const int tile = tile_lin - n * ntiles;
            float* dst = a.stats_partial + (((size_t)n * ntiles + tile) * a.Cout + co) * 2;
            dst[0] = s;
            dst[1] = q;
          }
        }
        // s_red is re-written only after the next item's two barriers, so no extra barrier is needed here
      }
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[r][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }  // last chunk of the tile
    VX_STAMP(5);
#ifdef VX_CONV_STAMPS
    ++st_iters;
#endif
    tile_lin = ntile; chunk = nchunk; have = nhave;
  }
#ifdef VX_CONV_STAMPS
  if (ka.dbg && blockIdx.y == 0 && (tid & 63) == 0) {
    unsigned long long* d = ka.dbg + ((size_t)blockIdx.x * NW + wave) * 8;
    for (int i = 0; i < 6; ++i) d[i] = st_sum[i];
    d[6] = st_iters;
  }
#endif
}

// ---------------------------------------------------------------------------------------------
// weight packing: torch (Cout, Cin, 3,3,3) -> [rowgroup][chunk][tap][nt][lane 64][CPL]
//   plain : row = cout, tap = (kz,ky,kx)                       (NT fixed per (Cin, Cout) by s16_config())
//   x-pair: row = dx*8 + cout, tap = (kz,ky,ix), value W[kx = ix - dx] or 0      (Cout == 8)
__global__ void pack_conv3d_k3_kernel(const float* __restrict__ w, float* __restrict__ out, int Cin, int Cout, int CB,
                                      int NT, int XP, int64_t total) {
  const int CPL = CB / 4;
  const int nchunks = Cin / CB;
  const int ntap = XP ? 36 : 27;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = i;
    const int j = r % CPL; r /= CPL;
    const int lane = r % 64; r /= 64;
    const int nt = r % NT; r /= NT;
    const int tap = r % ntap; r /= ntap;
    const int chunk = r % nchunks; r /= nchunks;
    const int rgrp = (int)r;
    const int row = (rgrp * NT + nt) * 16 + (lane & 15);
    const int ci = chunk * CB + (lane >> 4) * CPL + j;
    float v = 0.f;
    if (XP) {
      const int dx = row >> 3, co = row & 7;
      const int kzy = tap / 4, ix = tap % 4, kx = ix - dx;
      if (kx >= 0 && kx <= 2) v = w[((size_t)co * Cin + ci) * 27 + kzy * 3 + kx];
    } else if (row < Cout) {
      v = w[((size_t)row * Cin + ci) * 27 + tap];
    }
    out[i] = v;
  }
}

int vx_pack_conv3d_k3_mfma(const float* w_torch, float* w_packed, int Cin, int Cout, int64_t total, hipStream_t s) {
  const S16Cfg c = s16_config(Cin, Cout);
  int blocks = (int)((total + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(pack_conv3d_k3_kernel, dim3(blocks), dim3(256), 0, s, w_torch, w_packed, Cin, Cout, c.CB, c.NT, c.XP, total);
  VX_CHECK_LAUNCH("vx_pack_conv3d_k3");
  return VX_OK;
}

template <int CB, int NT, int TX, int TY, int TZ, int NW, int XP>
static int launch_conv(const ConvKArgs& ka, const Conv3dRoute& r, hipStream_t s) {
  constexpr int TXV = XP ? 2 * TX : TX;
  constexpr int NPOS = (TXV + 2) * (TY + 2) * (TZ + 2);  // = NPAR * NPP (HX is even for x-pair)
  constexpr int PLANE = CB == 16 ? ((NPOS + 15) / 16) * 16 : ((NPOS + 15) / 32) * 32 + 16;
  constexpr int IN_FLOATS = 4 * PLANE * (CB / 4);
  constexpr int W_FLOATS = (XP ? 36 : 27) * NT * 64 * (CB / 4);
  constexpr size_t lds = (size_t)(IN_FLOATS + W_FLOATS + NW * NT * 16 * 2) * sizeof(float);
  static_assert(lds <= 160 * 1024, "LDS budget");
  static bool attr_set = false;
  auto kern = conv3d_k3_mfma_kernel<CB, NT, TX, TY, TZ, NW, XP>;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds);
    if (e != hipSuccess) VX_FAIL((int)e, "vx_conv3d_k3: hipFuncSetAttribute(%zu B LDS): %s", lds, hipGetErrorString(e));
    attr_set = true;
  }
  const vx_conv3d_args& a = ka.a;
  // persistent workgroups: each loops over tiles with stride gridDim.x (prefetching the next tile's loads
  // while it computes); enough workgroups to fill every CU at the LDS-limited occupancy
  const int total_tiles = ka.tiles_x * ka.tiles_y * ka.tiles_z * a.N;
  const int ygroups = XP ? 1 : (a.Cout + 16 * NT - 1) / (16 * NT);
  int per_cu = (int)((160 * 1024) / lds) > 0 ? (int)((160 * 1024) / lds) : 1;
  if (per_cu * NW > 32) per_cu = 32 / NW;
  int gx = (256 * per_cu + ygroups - 1) / ygroups;
  if (gx > total_tiles) gx = total_tiles;
  dim3 grid((unsigned)gx, (unsigned)ygroups);
  static const char* kname = vx_conv3d_kname(r);
  vx_note_kernel(kname);
  hipLaunchKernelGGL(kern, grid, dim3(64 * NW), lds, s, ka);
  VX_CHECK_LAUNCH("vx_conv3d_k3");
  return VX_OK;
}

int vx_conv3d_mfma_launch(const Conv3dRoute& r, const vx_conv3d_args& a, hipStream_t s) {
  ConvKArgs ka;
  ka.a = a;
  ka.tiles_x = r.tiles_x; ka.tiles_y = r.tiles_y; ka.tiles_z = r.tiles_z;
  ka.nchunks = r.nchunks;
  ka.mx = r.mx; ka.my = r.my; ka.mz = r.mz;
  int unused;
  vx_conv_diag(VX_DIAG_NONE, &ka.dbg, &unused);
  switch (conv3d_key_of(r.p, r.np)) {
#define MFMA_CASE(...) case conv3d_key(__VA_ARGS__): return launch_conv<__VA_ARGS__>(ka, r, s);
    MFMA_INSTANCES(MFMA_CASE)
#undef MFMA_CASE
  }
  VX_FAIL(VX_E_SHAPE, "vx_conv3d_k3: no such instance of the fp32 tile kernel");
}
