// The MULTIPLYING role of conv3d_zc16_kernel (conv3d_zc16.hip), included once per evaluation of the fused up-convolution with
// ZC_CMP = 0 (the conv over the staged fine planes) or 1 (the composed up-convolution: the kernel's header).  Plain text inside
// the kernel's body, not a function or a lambda: wrapped in a generic lambda the instances at the 168-register limit spilled.
{
    constexpr bool CMP = ZC_CMP != 0;
    constexpr int RS = CMP ? 2 : 1;                  // output rows between two tiles of a wave
    const int c_py = (wave >> 1) & 1, c_px = wave & 1;
    const int lz = wave >> 2, xh = CMP ? 0 : (wave >> 1) & 1, ly0 = CMP ? c_py : (wave & 1) * R, x0 = 16 * xh;
    const bool late = wave >= NW / 2;
    // ---- compute-phase constants (byte offsets into the LDS image) ----
    // type-1 fragment of input row (slot, ly0 + j): lane (m, g) -> position x0 + m + kx, octet g & 1 (Cin = 16: kx = g >> 1;
    // Cin = 8: kx = g, the zero group g = 3 re-reads kx = 2: finite data under a zero weight)
    const int kxP = CIN == 16 ? (g >> 1) : (g < 2 ? g : 2);
    const int bP = (CIN == 16 ? (g & 1) * OCT_B : 0) + (ly0 * HX + x0 + m + kxP) * 16;
    const int bQ = (g & 1) * OCT_B + (ly0 * HX + x0 + m + 2) * 16;      // Cin = 16: the kx = 2 taps
    const unsigned char* wlane = s_w + lane * 16;

    // ---- epilogue constants: this lane stores voxel x0 + m of row ly0 + r, channels 4 g .. 4 g + 3 ----
    const int lx = CMP ? 2 * m + c_px : x0 + m, oc = 4 * g;      // (composed: row r of the wave is output row ly0 + 2 r)
    // (row r of the wave sits r output rows further: a scalar added to the store's soffset, one offset register per lane)
    // (composed: a dense float or planar output -- the route refuses out_xblk / out_split there, and their code is not compiled in)
    const bool xblk = !CMP && a.out_xblk != 0;
    unsigned ovoff0;
    if (xblk) {
      const int oxb = a.out_xblk;
      ovoff0 = (unsigned)((((lz * a.H + ly0) * (2 * a.W * 16)) + ((lx / oxb) * 2 + a.out_half) * oxb * 16 + (lx % oxb) * 16 + oc) * 4);
    } else {
      ovoff0 = (unsigned)((((lz * a.H + ly0) * a.W + lx) * a.out_pitch + a.out_coff + oc) * 4);
    }
    const unsigned orow = (unsigned)(a.W * (xblk ? 32 : a.out_pitch) * 4 * RS);   // bytes between two output rows of the wave
    // ONE hash round per item serves the wave's R rows (16 channels: a keep-word = 2 voxels, a half row = 8 words): lane i
    // computes word i & 7 of row i >> 3, a row's lanes fetch theirs with ds_bpermute.  Same bits as vx_drop_bits4(key, e).
    // Composed: a row's 16 voxels of one parity lie in 16 words -- lane i computes word i & 15 of row i >> 4.
    unsigned hword_l;
    if constexpr (CMP) {
      hword_l = (unsigned)((((lz * a.H + ly0 + 2 * (lane >> 4)) * a.W) >> 1) + (lane & 15));
    } else {
      const int rr_ = (lane >> 3) < R ? (lane >> 3) : 0;
      hword_l = (unsigned)((((lz * a.H + ly0 + rr_) * a.W + x0) >> 1) + (lane & 7));
    }
    const int out_voxf = xblk ? 32 : a.out_pitch;
    const size_t out_sample = (size_t)a.D * a.H * a.W * out_voxf;
    const bool f_lrelu = EPI == 3 ? a.act == VX_ACT_LRELU : EPI == 1;
    const bool f_relu = EPI == 3 && a.act == VX_ACT_RELU;

    f32x4 acc[R], accx[R];
    f32x4 accin[ACC ? R : 1];
    float ssum[4] = {0.f, 0.f, 0.f, 0.f}, ssq[4] = {0.f, 0.f, 0.f, 0.f};
    const unsigned avoff0 = ACC ? (unsigned)((((lz * a.H + ly0) * a.W + lx) * a.acc_pitch + oc) * 4) : 0u;
    const unsigned arow = ACC ? (unsigned)(a.W * a.acc_pitch * 4 * RS) : 0u;
    const size_t acc_sample = (size_t)a.D * a.H * a.W * (ACC ? a.acc_pitch : 0);

    // the multiply phase of the item whose first input plane (z0 - 1) sits in slot rb (item k of column ci)
    auto multiply = [&](int rb, int ci, int k) {
      if constexpr (ACC != 0) {
        int n_, ty_, tx_;
        col_of(ci, n_, ty_, tx_);
        const unsigned asoff = (unsigned)(((k * TZ) * a.H + ty_ * 8) * a.W + tx_ * 32) * (unsigned)a.acc_pitch * 4u;
        const __amdgpu_buffer_rsrc_t asrd = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(const_cast<float*>(kernarg()->a.acc_in) + (size_t)n_ * acc_sample), 0, VX_NUMREC, 0x00020000);
#pragma unroll
        for (int r = 0; r < R; ++r)
          accin[r] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(asrd, (int)avoff0, (int)(asoff + (unsigned)r * arow), 0));
      }
      const f32x4 bias4 = *reinterpret_cast<const f32x4*>(s_bias + oc);
      int sl[3];
#pragma unroll
      for (int kz = 0; kz < 3; ++kz) {
        int s_ = rb + lz + kz;
        if (s_ >= NZ) s_ -= NZ;
        sl[kz] = s_ * PLN_B;
      }
      // phases = groups of steps that share their row fragments.  Cin = 16: phases 0..2 (type 1, kz = phase) and 3 (the kx = 2 taps
      // of kz = 0 / 1) have three steps (ky) over 6 rows -- tile r of step ky reads row r + ky; phase 4 is the ONE step that holds
      // the kx = 2 taps of (kz = 2, ky = 0 / 1) as its two k-group pairs: its fragment of tile r mixes rows r and r + 1 by lane
      // (4 fragments, no reuse); phase 5 the half-empty step of (kz = 2, ky = 2): rows 2..5.  14 steps for 13.5 (round 5, second
      // version: the first ran the kz = 2 taps as three half-empty steps, 15).  Cin = 8: three phases of three steps.
      constexpr int NPH = CIN == 16 ? 6 : 3;
      auto ph_of = [](int t) { return t < 12 ? t / 3 : t - 8; };           // step -> phase
      auto ky_of = [](int t) { return t < 12 ? t % 3 : 0; };               // step -> row offset of tile r within the phase's rows
      auto nrows = [](int ph) { return ph < 4 ? R + 2 : R; };
      const unsigned char* rowp[NPH];
#pragma unroll
      for (int ph = 0; ph < NPH; ++ph) {
        if (ph < 3) rowp[ph] = s_img + bP + sl[ph];
        else if (ph == 3) rowp[ph] = s_img + bQ + ((g >> 1) ? sl[1] : sl[0]);
        else if (ph == 4) rowp[ph] = s_img + bQ + sl[2] + (g >> 1) * ROW_B;
        else rowp[ph] = s_img + bQ + sl[2] + 2 * ROW_B;
      }
#ifndef ZC_NO_PIPE
      if constexpr (!POOL)      // (the pooling instance holds 8 statistics registers + its window state across the loop: 168 + scratch)
      // ONE software pipeline over the NSTEP K-steps, 12 matrix instructions each.  Left alone hipcc sinks every ds_read_b128 to
      // just before its consumer (ds_read; s_waitcnt lgkmcnt(0..1); v_mfma).  Here every step requests, behind its own matrix
      // instructions and pinned there (sched_group_barrier), fragments of LATER steps:
      //   step (phase p, ky = 0): the weights of (p, 1) + rows 4, 5 of phase p          (needed at ky = 1 / ky = 2)
      //   step (p, 1):            the weights of (p, 2) + rows 0, 1 of phase p + 1
      //   step (p, 2):            the weights of (p + 1, 0) + rows 2, 3 of phase p + 1
      //   step 12 (phase 4):      the weights of step 13 + the four rows of phase 5
      // -- 0.5 reads per matrix instruction over the item.  Measured -2 .. -3.5 % (same-process A/B against the plain loop).
      {
        f16x8 rh[NPH][R + 2], rl[NPH][R + 2], wh[NSTEP], wl[NSTEP];
        auto ld_row = [&](int ph, int jr) {
          rh[ph][jr] = *reinterpret_cast<const f16x8*>(rowp[ph] + jr * ROW_B);
          rl[ph][jr] = *reinterpret_cast<const f16x8*>(rowp[ph] + jr * ROW_B + PREC_B);
        };
        auto ld_w = [&](int t) {
          wh[t] = *reinterpret_cast<const f16x8*>(wlane + t * 2048);
          wl[t] = *reinterpret_cast<const f16x8*>(wlane + t * 2048 + 1024);
        };
        ld_w(0);
#pragma unroll
        for (int jr = 0; jr < R; ++jr) ld_row(0, jr);
        __builtin_amdgcn_sched_group_barrier(0x100, 3 + 2 * R, 0);      // (+ the bias vector)
#pragma unroll
        for (int t = 0; t < NSTEP; ++t) {
          const int ph = ph_of(t), ky = ky_of(t);
          int nrd = 0;
          if (t + 1 < NSTEP) { ld_w(t + 1); nrd += 2; }
          if (t < 12) {
            if (ky == 0) { ld_row(ph, R); ld_row(ph, R + 1); nrd += 4; }
            else if (ph + 1 < NPH) { ld_row(ph + 1, 2 * (ky - 1)); ld_row(ph + 1, 2 * (ky - 1) + 1); nrd += 4; }
          } else if (t == 12) {
#pragma unroll
            for (int jr = 0; jr < R; ++jr) ld_row(5, jr);
            nrd += 2 * R;
          }
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const bool fresh = t == 0;      // the bias is the first product's C operand
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            acc[r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[t], rh[ph][r + ky], fresh ? (ACC ? zero : bias4) : acc[r], 0, 0, 0);
            accx[r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[t], rl[ph][r + ky], fresh ? zero : accx[r], 0, 0, 0);
            accx[r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[t], rh[ph][r + ky], accx[r], 0, 0, 0);
          }
#pragma unroll
          for (int i = 0; i < 3 * R; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            if (i < nrd) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          }
        }
        return;
      }
#endif
#pragma unroll
      for (int ph = 0; ph < NPH; ++ph) {
        f16x8 bh[R + 2], bl[R + 2];
#pragma unroll
        for (int jr = 0; jr < R + 2; ++jr) {
          if (jr < nrows(ph)) {
            bh[jr] = *reinterpret_cast<const f16x8*>(rowp[ph] + jr * ROW_B);
            bl[jr] = *reinterpret_cast<const f16x8*>(rowp[ph] + jr * ROW_B + PREC_B);
          }
        }
#pragma unroll
        for (int ky = 0; ky < (ph < 4 ? 3 : 1); ++ky) {
          const int step = ph < 4 ? ph * 3 + ky : 8 + ph;
          const f16x8 ah = *reinterpret_cast<const f16x8*>(wlane + step * 2048);
          const f16x8 al = *reinterpret_cast<const f16x8*>(wlane + step * 2048 + 1024);
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const bool fresh = ph == 0 && ky == 0;      // the bias is the first product's C operand
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            acc[r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh[r + ky], fresh ? (ACC ? zero : bias4) : acc[r], 0, 0, 0);
            accx[r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl[r + ky], fresh ? zero : accx[r], 0, 0, 0);
            accx[r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh[r + ky], accx[r], 0, 0, 0);
          }
        }
      }
    };

    // ---- composed: this wave's class of the composed weights, resident; the multiply phase of item k, visible with step jj ----
    // (the hi halves resident, 32 registers; the lo halves come from LDS per (a, c) group, requested a group ahead)
    f16x8 cwh[CMP ? 8 : 1];
    if constexpr (CMP) {
      const f16x8* wp = reinterpret_cast<const f16x8*>(a.up_fused) + (size_t)(wave * 8 * 2 * 64 + lane);
#pragma unroll
      for (int t = 0; t < 8; ++t) cwh[t] = wp[t * 128];
    }
    const unsigned char* cwl_lane = s_cwl + wave * 8 * 1024 + lane * 16;
    auto multiply_c = [&](int jj, int ci, int k) {
      if constexpr (CMP) {
        int n_, ty_, tx_;
        col_of(ci, n_, ty_, tx_);
        {
          const unsigned asoff = (unsigned)(((k * TZ) * a.H + ty_ * 8) * a.W + tx_ * 32) * (unsigned)a.acc_pitch * 4u;
          const __amdgpu_buffer_rsrc_t asrd = __builtin_amdgcn_make_buffer_rsrc(
              (void*)(const_cast<float*>(kernarg()->a.acc_in) + (size_t)n_ * acc_sample), 0, VX_NUMREC, 0x00020000);
#pragma unroll
          for (int r = 0; r < R; ++r)
            accin[r] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(asrd, (int)avoff0, (int)(asoff + (unsigned)r * arow), 0));
        }
        // border classes of this lane's voxels (0 first, 1 interior, 2 last): z of the item, x of the column, y per tile
        const int zg = k * TZ + lz, xg = tx_ * 32 + lx;
        const int bz = zg == 0 ? 0 : (zg == a.D - 1 ? 2 : 1), bx = xg == 0 ? 0 : (xg == a.W - 1 ? 2 : 1);
        const float* btl = s_btab + (bz * 9 + bx) * 16 + oc;
        // fragment of window (row jr + py, column m + px + c) of the slot of coarse plane k + pz - 1 + a = step jj - 2 + pz + a
        const unsigned char* cB = s_img + ((c_py * CW) + m + c_px) * 64 + g * 16;
        const int sb0 = ((jj + 2 + lz) & (CNS - 1)) * CSLOT_B, sb1 = ((jj + 3 + lz) & (CNS - 1)) * CSLOT_B;
        f16x8 fh[2], fl[2], wl[2][2];
        auto ld_wl = [&](int grp) {      // group (a, c) = grp: taps (a, 0, c), (a, 1, c)
          const int t0 = (grp >> 1) * 4 + (grp & 1);
          wl[grp & 1][0] = *reinterpret_cast<const f16x8*>(cwl_lane + t0 * 1024);
          wl[grp & 1][1] = *reinterpret_cast<const f16x8*>(cwl_lane + (t0 + 2) * 1024);
        };
        ld_wl(0);
        auto ld = [&](int i) {           // fragment i = (a, c, jr): 10 a + 5 c + jr
          const unsigned char* p = cB + (i >= 10 ? sb1 : sb0) + ((i % 5) * CW + ((i / 5) & 1)) * 64;
          fh[i & 1] = *reinterpret_cast<const f16x8*>(p);
          fl[i & 1] = *reinterpret_cast<const f16x8*>(p + CPREC_B);
        };
        ld(0);
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 20; ++i) {
          int nrd = 0;
          if (i + 1 < 20) { ld(i + 1); nrd += 2; }     // (requested behind this fragment's matrix instructions, pinned there)
          if (i % 5 == 2 && i / 5 + 1 < 4) { ld_wl(i / 5 + 1); nrd += 2; }
          const int ta = i / 10, tc = (i / 5) & 1, jr = i % 5;
          const f16x8 bh = fh[i & 1], bl = fl[i & 1];
          // tile jr with b = 0 and tile jr - 1 with b = 1: two independent accumulator chains, interleaved
          const int t0 = ta * 4 + tc, t1 = ta * 4 + 2 + tc;
          const bool d0 = jr < R, d1 = jr >= 1;
          const bool fresh = i == jr;      // (a, c) = (0, 0), b = 0: the tile's first product
          f32x4 c0 = zero;
          if (d0 && fresh) {
            const int yg = ty_ * 8 + 2 * jr + ly0;
            const int by = yg == 0 ? 0 : (yg == a.H - 1 ? 2 : 1);
            c0 = *reinterpret_cast<const f32x4*>(btl + by * 48);
          }
          if (d0) acc[jr] = __builtin_amdgcn_mfma_f32_16x16x32_f16(cwh[t0], bh, fresh ? c0 : acc[jr], 0, 0, 0);
          if (d1) acc[jr - 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(cwh[t1], bh, acc[jr - 1], 0, 0, 0);
          if (d0) accx[jr] = __builtin_amdgcn_mfma_f32_16x16x32_f16(cwh[t0], bl, fresh ? zero : accx[jr], 0, 0, 0);
          if (d1) accx[jr - 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(cwh[t1], bl, accx[jr - 1], 0, 0, 0);
          if (d0) accx[jr] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[(i / 5) & 1][0], bh, accx[jr], 0, 0, 0);
          if (d1) accx[jr - 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[(i / 5) & 1][1], bh, accx[jr - 1], 0, 0, 0);
          const int nmm = 3 * ((d0 ? 1 : 0) + (d1 ? 1 : 0));
#pragma unroll
          for (int q = 0; q < nmm; ++q) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            if (q < nrd) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          }
        }
      }
    };

    // ---- epilogue state of THIS wave (column it is storing) ----
    int e_ci = -1, e_n = 0, e_ty = 0, e_tx = 0;
    vx_dkey e_key = {0u, 0u};

    auto epilogue = [&](int ci, int k) {
      if (ci != e_ci) {
        e_ci = ci;
        col_of(ci, e_n, e_ty, e_tx);
        if (EPI == 1 || EPI == 4) e_key = vx_drop_key(seed_out, kernarg()->a.drop_layer, (uint32_t)e_n);
      }
      const unsigned vox0 = (unsigned)(((k * TZ) * a.H + e_ty * 8) * a.W + e_tx * 32);
      const unsigned osoff = xblk ? (unsigned)((((k * TZ) * a.H + e_ty * 8) * (2 * a.W * 16) + e_tx * 32 * 32) * 4)
                                        : vox0 * (unsigned)a.out_pitch * 4u;
      const int hbp = CMP ? 4 * m : 4 * (m >> 1);                 // (recomputed per item: two registers less across the matrix loop)
      const unsigned hsh = (unsigned)((CMP ? c_px : (m & 1)) * 16 + oc);
      constexpr int HBR = CMP ? 64 : 32;                          // bytes of lane address between two rows' words
      const bool e_hash = (EPI == 1) || (EPI == 4 && a.drop_mode == VX_DROP_HASH);
      const uint32_t hw_item = e_hash ? vx_drop_word(e_key, (vox0 >> 1) + hword_l) : 0u;
      const __amdgpu_buffer_rsrc_t osrd = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(reinterpret_cast<char*>(kernarg()->a.out) + (size_t)e_n * out_sample * 4), 0, VX_NUMREC, 0x00020000);
      float pl_max[4];
      uint32_t pl_any = 0u;
      __amdgpu_buffer_rsrc_t psrd = osrd, fsrd = osrd;
      if constexpr (POOL) {
        const auto kp = kernarg();
        const size_t pvs = (size_t)a.D * (a.H >> 1) * (a.W >> 1);      // pooled (y, x) voxels per sample
        psrd = __builtin_amdgcn_make_buffer_rsrc((void*)(kp->a.pool_out + (size_t)e_n * pvs * 16), 0, VX_NUMREC, 0x00020000);
        fsrd = __builtin_amdgcn_make_buffer_rsrc((void*)(kp->a.pool_flags + (size_t)e_n * pvs * 4), 0, VX_NUMREC, 0x00020000);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        f32x4 v;       // main + cross * 2^-11: one fma per element (exact scaling)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = fmaf(accx[r][j], 1.0f / 2048.f, acc[r][j]);
        if constexpr (ACC != 0) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] += accin[r][j];
        }
        if (STATS) {
#pragma unroll
          for (int j = 0; j < 4; ++j) { ssum[j] += v[j]; ssq[j] = fmaf(v[j], v[j], ssq[j]); }
        }
        if constexpr (POOL) {
          uint32_t bits = 0xFu;
          if (e_hash) bits = ((uint32_t)__builtin_amdgcn_ds_bpermute(hbp + HBR * r, (int)hw_item) >> hsh) & 0xFu;
          pl_any = (r & 1) ? (pl_any | (~bits & 0xFu)) : (~bits & 0xFu);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float kept = ((bits >> j) & 1u) ? v[j] : -INFINITY;
            pl_max[j] = (r & 1) ? fmaxf(pl_max[j], kept) : kept;
          }
        }
        if (f_lrelu) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.01f * v[j]);
        } else if (f_relu) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j], 0.f);
        }
        if (EPI == 1) {
          const uint32_t bits = ((uint32_t)__builtin_amdgcn_ds_bpermute(hbp + HBR * r, (int)hw_item) >> hsh) & 0xFu;
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] *= __uint_as_float((bits << (30 - j)) & 0x40000000u);
        }
        if (!STATS) rmax = fmaxf(fmaxf(rmax, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
        u32x4 sv = __builtin_bit_cast(u32x4, v);
        if (EPI == 1 || EPI == 3) {
          if constexpr (PLN) {
            // the consumer stages by LDS-DMA: its image rows are [octet][hi | lo][x][8 halves] -- this lane's 4 channels are one half
            // of a 16-byte entry of the hi plane and of the lo plane of octet g >> 1 (the lane pair g, g ^ 1 fills the entry)
            typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
            f16x4 hi, lo;
            vx_split4_s(v, hi, lo);
            const unsigned rowB = (unsigned)a.W * 64u, plB = (unsigned)a.W * 16u;
            int ln = lane;
            asm volatile("" : "+v"(ln));          // (keeps this address arithmetic inside the epilogue: one register less across the matrix loop)
            const int g_ = ln >> 4, m_ = ln & 15;
            const unsigned pvo = (unsigned)(lz * a.H + ly0) * rowB + (unsigned)((g_ >> 1) * 2) * plB + (unsigned)(CMP ? 2 * m_ + c_px : x0 + m_) * 16u + (unsigned)(g_ & 1) * 8u;
            const unsigned pso = (unsigned)((k * TZ) * a.H + e_ty * 8 + r * RS) * rowB + (unsigned)(e_tx * 32) * 16u;
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, hi), osrd, (int)pvo, (int)pso, 0);
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, lo), osrd, (int)pvo, (int)(pso + plB), 0);
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_nop 3" ::: "memory");      // (the store-data hazard with an SGPR soffset, below)
            __builtin_amdgcn_sched_barrier(0);
            continue;
          }
          if (!CMP && a.out_split) {   // the consumer is the fused up-convolution: hand the piece over as the fp16 pairs it multiplies
            typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
            f16x4 hi, lo;
            vx_split4_s(v, hi, lo);      // (plain instructions: packed fp32 beside the partner wave's matrix stream costs three)
            const u32x2 h2 = __builtin_bit_cast(u32x2, hi), l2 = __builtin_bit_cast(u32x2, lo);
            sv = (u32x4){h2[0], h2[1], l2[0], l2[1]};
          }
        }
        __builtin_amdgcn_raw_buffer_store_b128(sv, osrd, (int)ovoff0, (int)(osoff + (unsigned)r * orow), 0);
        // gfx950 store-data hazard with an SGPR soffset (conv3d_mfma.hip)
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop 3" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (POOL) {
          if (r & 1) {
            // a row pair is complete.  The x-neighbour (same channels) is the adjacent lane: quad_perm [1, 0, 3, 2]; even lanes
            // store the window of their z-plane: pool_out [N][D][H/2][W/2][16], pool_flags [N][D][H/2][W/2][4] (the flag word of a
            // 16-byte piece sits at a quarter of the piece's byte offset); odd lanes are steered out of the descriptor's range
            const int Hp = a.H >> 1, Wp = a.W >> 1;
            u32x4 mx;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int o = __builtin_amdgcn_update_dpp(0, __float_as_int(pl_max[j]), 0xB1, 0xF, 0xF, true);
              mx[j] = __float_as_uint(fmaxf(pl_max[j], __int_as_float(o)));
            }
            const uint32_t oany = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)pl_any, 0xB1, 0xF, 0xF, true);
            // lane part: ((lz Hp + ly0 / 2) Wp + lx / 2) 64 + 16 g bytes; scalar part: item, column, row pair
            const unsigned pvo = (m & 1) ? VX_OOB : (unsigned)((((lz * Hp + (ly0 >> 1)) * Wp + (lx >> 1)) * 16 + oc) * 4);
            const unsigned pso = (unsigned)(((((k * TZ) * Hp + e_ty * 4 + (r >> 1)) * Wp) + e_tx * 16) * 64);
            __builtin_amdgcn_raw_buffer_store_b128(mx, psrd, (int)pvo, (int)pso, 0);
            __builtin_amdgcn_raw_buffer_store_b32(pl_any | oany, fsrd, (int)((m & 1) ? VX_OOB : (pvo >> 2)), (int)(pso >> 2), 0);
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_nop 3" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
      if (STATS && k == KZ - 1) {
        // the column is complete for this wave: sum over its 16 voxel columns and leave the 4 x 2 values of row group g
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float s = ssum[j], q = ssq[j];
#pragma unroll
          for (int rot = 8; rot >= 1; rot >>= 1) { s += vx_row_ror(s, rot); q += vx_row_ror(q, rot); }
          if (m == 0) {
            s_red[(wave * 16 + g * 4 + j) * 2 + 0] = s;
            s_red[(wave * 16 + g * 4 + j) * 2 + 1] = q;
          }
          ssum[j] = 0.f; ssq[j] = 0.f;
        }
      }
    };

    // statistics of a complete column: entry 0 of the column's block is real, the other stat_epc - 1 are zero
    // (vx_instnorm_finalize sums vx_conv3d_k3_tiles_for entries per sample)
    auto flush_col = [&](int ci) {
      int n, ty, tx;
      col_of(ci, n, ty, tx);
      const auto kp = kernarg();
      const int epc = kp->stat_epc;
      const int ntile = cps * epc;
      float* dst = kp->a.stats_partial + (((size_t)n * ntile + (size_t)(ty * ka.tiles_x + tx) * epc) * 16) * 2;
      if (tid < 16) {
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
          s += s_red[(w * 16 + tid) * 2 + 0];
          q += s_red[(w * 16 + tid) * 2 + 1];
        }
        dst[tid * 2 + 0] = s;
        dst[tid * 2 + 1] = q;
      }
      for (int i = 32 + tid; i < epc * 32; i += 256) {
        if (tid < 256) dst[i] = 0.f;
      }
    };

    Cur cx = {0, 0};
    int j = 0;                                   // S_j = cx;  its slot group is j % 3
    int grp_x = 0;
    int prev_ci = -1, prev_k = 0;                // waves 4..7: the item still to store
    int fl_ci = -1, fl_at = 0;                   // column whose statistics are complete after barrier fl_at
    while (cx.ci < ncol_wg) {
      __syncthreads();
      ZC_STAMP(0);
      if (STATS && fl_ci >= 0 && j >= fl_at && !late) { flush_col(fl_ci); fl_ci = -1; }
      const bool comp = cx.s >= 1;
      const int item_k = cx.s - 1;
      int grp_c = grp_x + 1; if (grp_c == 3) grp_c = 0;
      const int rb = (grp_x == 0 ? 2 : grp_x - 1) * TZ + (TZ - 2);           // first plane of the item: group of S_{j-1}, plane TZ - 2
      if (late) {
        if (prev_ci >= 0 && !(ZC_ABL & 2)) { epilogue(prev_ci, prev_k); prev_ci = -1; }
        ZC_STAMP(2);
        if (comp) { if (!(ZC_ABL & 1)) { if constexpr (CMP) multiply_c(j, cx.ci, item_k); else multiply(rb, cx.ci, item_k); } prev_ci = cx.ci; prev_k = item_k; }
        ZC_STAMP(1);
      } else {
        if (comp && !(ZC_ABL & 1)) { if constexpr (CMP) multiply_c(j, cx.ci, item_k); else multiply(rb, cx.ci, item_k); }
        ZC_STAMP(1);
        if (comp && !(ZC_ABL & 2)) epilogue(cx.ci, item_k);
        ZC_STAMP(2);
      }
      if (STATS && comp && item_k == KZ - 1) { fl_ci = cx.ci; fl_at = j + 2; }
#ifdef VX_CONV_STAMPS
      ++st_iters;
#endif
      advance(cx);
      grp_x = grp_c;
      ++j;
    }
    if (late && prev_ci >= 0) epilogue(prev_ci, prev_k);
    if (STATS) {
      __syncthreads();
      if (fl_ci >= 0 && !late) flush_col(fl_ci);
    }
}
