// The main loop of gather_gemm_f32_glds_kernel<..., EMU = 1>: fp32 products on the bf16 matrix pipe (split3, conv_gemm_glds.inc).
// Textually included in the kernel's tile loop, in place of the chunk() loop of the fp32-MFMA form: same stages, same DMA
// issue / counted vmcnt wait / barrier at the top of a chunk, same accumulators and epilogue.  (KTJ = tile columns of the wave in
// the main loop: TJ of the epilogue unless the waves are K-partitioned, WGK = 2 -- then each wave works on ONE pair of the chunk.)
//
// A chunk of 32 k is two PAIRS of super-steps (16 k each = one bf16 MFMA step): read, split and multiply a pair at a time, the
// second pair's reads in flight behind the first pair's MFMAs.  What overlaps the VALU instructions of one wave's split with
// MFMAs is the other wave of the SIMD (two blocks per CU).  Tried and measured slower on rb1 / rb2 of config #2 (DESIGN.md
// section 4; the second in profiles/r04_emu2_probe.txt): the same loop software-pipelined by hand -- the split of the next pair
// behind the MFMAs of this one, groups fixed by sched_barrier -- at two blocks per CU (the two live split sets spill, and a
// scratch reload's `s_waitcnt vmcnt(0)` drains the LDS-DMA queue) and at one block per CU with 512 registers (one wave per
// SIMD: the split's VALU instructions cost ~7 cycles each beside MFMAs, so a 64 x 64 wave tile -- 32 half splits against 24
// MFMAs per pair -- stays VALU-bound with nobody to fill the matrix pipe meanwhile).
{
  static_assert(!xform, "EMU: plain operand forms");
  constexpr int NM = 6 * TI * KTJ;                         // MFMAs of a pair
  constexpr int NP = 4 * (TI + KTJ);                       // split3_pair pieces of a pair (four per fragment)
  f32x4v ea[2][TI], eb[2][w_nk ? KTJ : 1];
  float ek[2][w_nk ? 1 : KTJ][4];
  Split3 sa[2 / WGK][TI], sb[2 / WGK][KTJ];                // one split set per pair the wave works on

  auto top = [&](int it, auto curc) {
    constexpr int cur = decltype(curc)::value;
    const int younger = total - 1 - it < NSTAGE - 2 ? total - 1 - it : NSTAGE - 2;
    if (NSTAGE >= 4 && younger == 2) wait_vmcnt<2 * LPS>();
    else if (NSTAGE >= 3 && younger == 1) wait_vmcnt<LPS>();
    else wait_vmcnt<0>();
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (it + NSTAGE - 1 < total) issue(std::integral_constant<int, (cur + NSTAGE - 1) % NSTAGE>{});
  };
  // the lane's eight k of pair p (super-steps 2 p and 2 p + 1) of the stage in buffer cur (K-partitioned: p = 0 is the wave's
  // own pair, the offsets hold its place in the chunk)
  auto reads = [&](auto curc, auto pc) {
    constexpr unsigned stage_off = (unsigned)(decltype(curc)::value * STAGE_BYTES);
    constexpr int p = decltype(pc)::value;
    static_for<2>([&](auto sc) {
      constexpr int s = decltype(sc)::value, q = 2 * p + s;
#pragma unroll
      for (int i = 0; i < TI; ++i) lds_frag_f4<0>(ea[s][i], lds_base + stage_off + aoff[i][q]);
      if constexpr (w_nk) {
#pragma unroll
        for (int j = 0; j < KTJ; ++j) lds_frag_f4<0>(eb[s][w_nk ? j : 0], lds_base + stage_off + boff[j][w_nk ? q : 0]);
      } else {
#pragma unroll
        for (int j = 0; j < KTJ; ++j) {
          lds_frag_f1<(8 * q + 0) * B_ROWB>(ek[s][w_nk ? 0 : j][0], lds_base + stage_off + boff[j][0]);
          lds_frag_f1<(8 * q + 1) * B_ROWB>(ek[s][w_nk ? 0 : j][1], lds_base + stage_off + boff[j][0]);
          lds_frag_f1<(8 * q + 2) * B_ROWB>(ek[s][w_nk ? 0 : j][2], lds_base + stage_off + boff[j][0]);
          lds_frag_f1<(8 * q + 3) * B_ROWB>(ek[s][w_nk ? 0 : j][3], lds_base + stage_off + boff[j][0]);
        }
      }
    });
  };
  auto fence_e = [&]() {
    MOPOE_DEVICE_ASM("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int i = 0; i < TI; ++i) pin_reg(ea[s][i]);
      if constexpr (w_nk) {
#pragma unroll
        for (int j = 0; j < KTJ; ++j) pin_reg(eb[s][w_nk ? j : 0]);
      } else {
#pragma unroll
        for (int j = 0; j < KTJ; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) pin_reg(ek[s][w_nk ? 0 : j][e]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  // piece u of the pair in ea / eb / ek -> word u % 4 of fragment u / 4 of split set d
  auto piece = [&](auto uc, auto dc) {
    constexpr int u = decltype(uc)::value, d = decltype(dc)::value;
    constexpr int f = u / 4, w = u % 4, s = w / 2, e0 = 2 * (w % 2);
    unsigned h, m, l;
    if constexpr (f < TI) {
      split3_pair(ea[s][f][e0], ea[s][f][e0 + 1], h, m, l);
      sa[d][f].h[w] = h; sa[d][f].m[w] = m; sa[d][f].l[w] = l;
    } else {
      constexpr int j = f - TI;
      if constexpr (w_nk) split3_pair(eb[s][w_nk ? j : 0][e0], eb[s][w_nk ? j : 0][e0 + 1], h, m, l);
      else split3_pair(ek[s][w_nk ? 0 : j][e0], ek[s][w_nk ? 0 : j][e0 + 1], h, m, l);
      sb[d][j].h[w] = h; sb[d][j].m[w] = m; sb[d][j].l[w] = l;
    }
  };
  // MFMA t of split set d, term-major (consecutive MFMAs go to different accumulators)
  auto mfma_t = [&](auto tc, auto dc) {
    constexpr int t = decltype(tc)::value, d = decltype(dc)::value;
    constexpr int term = t / (TI * KTJ), tile = t % (TI * KTJ), i = tile % TI, j = tile / TI;
    mfma_split_term<term>(acc[i][j], sa[d][i], sb[d][j]);
  };
  using E0 = std::integral_constant<int, 0>; using E1 = std::integral_constant<int, 1>;
  using S1 = std::integral_constant<int, 2 / WGK - 1>;     // split set of the second pair
  auto all_pieces = [&](auto dc) { static_for<NP>([&](auto uc) { piece(uc, dc); }); };
  auto all_mfma = [&](auto dc) { static_for<NM>([&](auto tc) { mfma_t(tc, dc); }); };
  auto chunk2 = [&](int it, auto curc) {
    top(it, curc);
    reads(curc, E0{});
    fence_e();
    all_pieces(E0{});
    __builtin_amdgcn_sched_barrier(0);
    reads(curc, E1{});               // in flight behind the MFMAs of the first pair
    all_mfma(E0{});
    __builtin_amdgcn_sched_barrier(0);
    fence_e();
    all_pieces(S1{});
    __builtin_amdgcn_sched_barrier(0);
    all_mfma(S1{});
    __builtin_amdgcn_sched_barrier(0);
  };
  // K-partitioned: the wave's one pair of the chunk.  Nothing of its own to put behind the MFMAs -- the next reads need the next
  // barrier -- so what covers the reads and the split is the other waves of the SIMD, as in the first pair above
  auto chunk1 = [&](int it, auto curc) {
    top(it, curc);
    reads(curc, E0{});
    fence_e();
    all_pieces(E0{});
    __builtin_amdgcn_sched_barrier(0);
    all_mfma(E0{});
    __builtin_amdgcn_sched_barrier(0);
  };
  auto chunk_e = [&](int it, auto curc) {
    if constexpr (WGK == 2) chunk1(it, curc);
    else chunk2(it, curc);
  };
  int it = 0;
  while (it < total) {
    chunk_e(it, std::integral_constant<int, 0>{});
    if (++it >= total) break;
    chunk_e(it, std::integral_constant<int, 1>{});
    if (++it >= total) break;
    if constexpr (NSTAGE >= 3) { chunk_e(it, std::integral_constant<int, 2 % NSTAGE>{}); if (++it >= total) break; }
    if constexpr (NSTAGE >= 4) { chunk_e(it, std::integral_constant<int, 3 % NSTAGE>{}); ++it; }
  }
}
