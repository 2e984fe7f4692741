// gather_gemm_f32_glds_kernel: the fp32 implicit-GEMM main loop on LDS-DMA (`buffer_load_dwordx4 ... lds`), the fp32
// counterpart of conv_gemm_bf16_glds.inc.  Textually included by conv_gemm.hip (same GemmArgs, same row-major epilogue).
//
// Why (round 3).  The register-staged fp32 kernel keeps ONE chunk of 16 (or 32) K elements in flight per block: on the
// large layers fp32 MFMA time (64 cycles per 32x32x2 instruction) covers that, which is why they sit at 0.65-0.73 of the
// fp32-MFMA peak; on the deep layers of the networks (4x4 / 8x8 maps, the 1-D text layers: M of 64 ... 4096 rows, K of
// 2048 ... 10240, a few tens of blocks per launch after the split of the reduction) every chunk is a dependent
// load -> barrier -> few MFMAs round trip of ~1.2 us, and the launches run at 25-50 TFLOP/s (profiles/r02_layers_c2.txt:
// 3-4 ms of the 12.6 ms of conv time per C2 step).  Here a stage is a 32-deep chunk that arrives by DMA straight into LDS
// (no VGPRs, no ds_write), and NSTAGE buffers keep NSTAGE-1 stages in flight behind a counted `s_waitcnt vmcnt(N)` and a raw
// `s_barrier`: the round trip is paid once per tile, not once per chunk.
//
// LDS images, as the DMA leaves them (wave-uniform base + lane * 16, no padding possible):
//   K-contiguous operands (activations [row][32 k]; input-gradient weights [n][32 k]): 128-byte rows, the 16-byte slot c of row
//     r holds the row's logical chunk c ^ ((r >> 1) & 7) (permutation applied to the per-lane SOURCE address and again on the
//     read): the 16 rows of a ds_read_b128 lane group cover all 16 slots of the bank row -- conflict-free.
//   K-strided operand (forward weights [32 k][BN n]): rows of BN floats as they lie in memory, read with ds_read_b32 (32
//     consecutive lanes = 32 consecutive columns of one k row): conflict-free without a permutation.
// MFMA K order.  v_mfma_f32_32x32x2_f32 takes k = 0 from lanes 0-31 and k = 1 from lanes 32-63.  Any bijection of the
// chunk's 32 k values onto (instruction, lane half) is legal as long as both operands use the same one: lane half h of the
// four instructions of "super-step" q multiplies k = 8 q + 4 h + {0, 1, 2, 3}, so that ONE ds_read_b128 of a K-contiguous
// fragment (4 consecutive floats of the lane's row) feeds four MFMAs.  The sums are the same fp32 fma chains as before in a
// different order of the 32 products of a chunk (fp32 summation order is not part of the parity contract: tests compare
// against the emulation at 2e-4 of the tensor scale, as for every other tile).
typedef float f32x4v __attribute__((ext_vector_type(4)));

template <int OFF>
__device__ __forceinline__ void lds_frag_f4(f32x4v& r, unsigned addr) {
  static_assert(OFF >= 0 && OFF < 65536, "ds offset field");
  MOPOE_DEVICE_ASM("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF) : "memory");
}
template <int OFF>
__device__ __forceinline__ void lds_frag_f1(float& r, unsigned addr) {
  static_assert(OFF >= 0 && OFF < 65536, "ds offset field");
  MOPOE_DEVICE_ASM("ds_read_b32 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF) : "memory");
}

// four consecutive 1-KB rows of 16 bytes per lane (the accumulator exchange of the K-partitioned waves); valid on return
__device__ __forceinline__ void lds_load_x4(u32x4& a, u32x4& b, u32x4& c, u32x4& d, unsigned addr) {
  MOPOE_DEVICE_ASM("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:1024\n\tds_read_b128 %2, %4 offset:2048\n\tds_read_b128 %3, %4 offset:3072\n\ts_waitcnt lgkmcnt(0)"
                   : "=&v"(a), "=&v"(b), "=&v"(c), "=&v"(d) : "v"(addr) : "memory");
}

// ---- EMU: the fp32 products on the bf16 matrix pipe (round 4) ------------------------------------------------------------------
// An fp32 number is the exact sum of three bf16 numbers: h = bf16(a), m = bf16(a - h), l = a - h - m (round-to-nearest-even
// conversions; a - h has at most 16 significant bits and |a - h| <= 2^-8 |a|, a - h - m at most 8: l is exact).  The product of
// two bf16 numbers is exact in fp32, so a b = sum of nine exact products, accumulated in fp32 by the bf16 MFMA exactly as the
// fp32 MFMA accumulates its own products.  Six of the nine are issued: hh, hm, mh, mm, hl, lh.  The three left out (m l, l m, l l)
// are bounded by 2^-24 |a b| each in the worst case (|m| <= 2^-8 |a|, |l| <= 2^-16 |b|) and are zero-mean with a typical size of
// 2^-28 |a b| -- below the 2^-24 rounding of the fp32 product itself, which v_mfma_f32_32x32x2_f32 commits once per product and this
// path does not commit at all (tests/test_hip_ops_gpu.py::test_f32_products_on_the_bf16_pipe measures both against fp64: the
// split form is the more accurate one).  One v_mfma_f32_32x32x16_bf16 is 8 passes for 16 k, the fp32 instruction 16 passes for
// 2 k: six of the former replace eight of the latter, 192 matrix-pipe cycles instead of 512 per 32 x 32 x 16 block, paid for
// with ~5 VALU instructions per operand element (v_cvt_pk_bf16_f32, two unpacks, v_pk_add_f32, twice).
// Non-finite operands: inf - bf16(inf) is NaN, so an infinite activation yields NaN where the fp32 MFMA yields inf (the train
// step treats either as a non-finite loss); |a| within 2^-9 of FLT_MAX rounds h to inf.
typedef __bf16 e_bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 e_bf16x8 __attribute__((ext_vector_type(8)));
typedef float e_f32x2 __attribute__((ext_vector_type(2)));
struct Split3 { u32x4 h, m, l; };                         // eight bf16 each: k slot 2 t in the low half of word t

__device__ __forceinline__ void split3_pair(float a0, float a1, unsigned& h, unsigned& m, unsigned& l) {
#if defined(MOPOE_DBG_EMU_NOSPLIT)    // timing build: no VALU work (wrong products)
  h = __float_as_uint(a0); m = __float_as_uint(a1); l = h;
  return;
#endif
  // (the subtractions in assembly: left to the compiler they are packed into v_pk_add_f32, which beside MFMAs costs three
  // times a v_sub_f32 -- MI355X_MICROARCH.md, 'price of one filler beside MFMAs')
  const e_f32x2 a = {a0, a1};
  h = __builtin_bit_cast(unsigned, __builtin_convertvector(a, e_bf16x2));
  float r0 = 0.f, r1 = 0.f, q0 = 0.f, q1 = 0.f;
  MOPOE_DEVICE_ASM_PURE("v_sub_f32 %0, %1, %2" : "=v"(r0) : "v"(a0), "v"(h << 16));
  MOPOE_DEVICE_ASM_PURE("v_sub_f32 %0, %1, %2" : "=v"(r1) : "v"(a1), "v"(h & 0xffff0000u));
  const e_f32x2 r = {r0, r1};
  m = __builtin_bit_cast(unsigned, __builtin_convertvector(r, e_bf16x2));
  MOPOE_DEVICE_ASM_PURE("v_sub_f32 %0, %1, %2" : "=v"(q0) : "v"(r0), "v"(m << 16));
  MOPOE_DEVICE_ASM_PURE("v_sub_f32 %0, %1, %2" : "=v"(q1) : "v"(r1), "v"(m & 0xffff0000u));
  const e_f32x2 r2 = {q0, q1};
  l = __builtin_bit_cast(unsigned, __builtin_convertvector(r2, e_bf16x2));
}
// the same in two halves (five and six VALU instructions: what fits behind one MFMA of the same wave): h and the remainders ...
__device__ __forceinline__ void split3_first(float a0, float a1, unsigned& h, float& r0, float& r1) {
  const e_f32x2 a = {a0, a1};
  h = __builtin_bit_cast(unsigned, __builtin_convertvector(a, e_bf16x2));
  MOPOE_DEVICE_ASM_PURE("v_sub_f32 %0, %1, %2" : "=v"(r0) : "v"(a0), "v"(h << 16));
  MOPOE_DEVICE_ASM_PURE("v_sub_f32 %0, %1, %2" : "=v"(r1) : "v"(a1), "v"(h & 0xffff0000u));
}
// ... then m and l from the remainders
__device__ __forceinline__ void split3_second(float r0, float r1, unsigned& m, unsigned& l) {
  const e_f32x2 r = {r0, r1};
  m = __builtin_bit_cast(unsigned, __builtin_convertvector(r, e_bf16x2));
  float q0 = 0.f, q1 = 0.f;
  MOPOE_DEVICE_ASM_PURE("v_sub_f32 %0, %1, %2" : "=v"(q0) : "v"(r0), "v"(m << 16));
  MOPOE_DEVICE_ASM_PURE("v_sub_f32 %0, %1, %2" : "=v"(q1) : "v"(r1), "v"(m & 0xffff0000u));
  const e_f32x2 q = {q0, q1};
  l = __builtin_bit_cast(unsigned, __builtin_convertvector(q, e_bf16x2));
}
// v0 = the lane's four k of an even super-step, v1 = of the odd one after it: the lane's eight k slots of one bf16 MFMA
__device__ __forceinline__ Split3 split3(const float (&v0)[4], const float (&v1)[4]) {
  unsigned h[4], m[4], l[4];
  split3_pair(v0[0], v0[1], h[0], m[0], l[0]);
  split3_pair(v0[2], v0[3], h[1], m[1], l[1]);
  split3_pair(v1[0], v1[1], h[2], m[2], l[2]);
  split3_pair(v1[2], v1[3], h[3], m[3], l[3]);
  Split3 s;
  s.h = u32x4{h[0], h[1], h[2], h[3]};
  s.m = u32x4{m[0], m[1], m[2], m[3]};
  s.l = u32x4{l[0], l[1], l[2], l[3]};
  return s;
}
__device__ __forceinline__ Split3 split3(const f32x4v& v0, const f32x4v& v1) {
  const float a[4] = {v0[0], v0[1], v0[2], v0[3]}, b[4] = {v1[0], v1[1], v1[2], v1[3]};
  return split3(a, b);
}
__device__ __forceinline__ f32x16 mfma_bf16(const u32x4& a, const u32x4& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(e_bf16x8, a), __builtin_bit_cast(e_bf16x8, b), c, 0, 0, 0);
}
// acc += A B for one 32 x 32 tile and 16 k: small terms first
__device__ __forceinline__ void mfma_split6(f32x16& acc, const Split3& a, const Split3& b) {
  acc = mfma_bf16(a.h, b.l, acc);
  acc = mfma_bf16(a.l, b.h, acc);
  acc = mfma_bf16(a.m, b.m, acc);
  acc = mfma_bf16(a.h, b.m, acc);
  acc = mfma_bf16(a.m, b.h, acc);
  acc = mfma_bf16(a.h, b.h, acc);
}
// term TERM of the six, small terms first: hl, lh, mm, hm, mh, hh
template <int TERM>
__device__ __forceinline__ void mfma_split_term(f32x16& acc, const Split3& a, const Split3& b) {
#if defined(MOPOE_DBG_EMU_NOMFMA)
  MOPOE_DEVICE_ASM("" :: "v"(a.h), "v"(a.m), "v"(a.l), "v"(b.h), "v"(b.m), "v"(b.l));
#else
  const u32x4& x = TERM == 1 ? a.l : ((TERM == 2 || TERM == 4) ? a.m : a.h);
  const u32x4& y = TERM == 0 ? b.l : ((TERM == 2 || TERM == 3) ? b.m : b.h);
  acc = mfma_bf16(x, y, acc);
#endif
}
// ties a register to this point of the instruction stream (no instruction): what is read from it comes after
template <typename T>
__device__ __forceinline__ void pin_reg(T& r) { MOPOE_DEVICE_ASM("" : "+v"(r)); }

// SPEC: 1 forward, plain operand (weights K-strided)   3 input gradient (weights K-contiguous)
//       2 forward with BN -> ReLU on the gathered operand: weights by DMA, activations through registers.  The raw rows of a
//         stage are requested R iterations before they are transformed and written into the LDS buffer that has just become
//         free (R = 1 with two buffers, R = 2 with four: the small tile of the deep layers needs more than one 0.5-us
//         iteration to cover a load), and sit there NSTAGE - 1 further iterations like a DMA'd stage
//   WGK: 1 = every wave of the block walks all of k; 2 = K-partitioned (EMU only): the block's waves are WGM x WGNK x 2, wave
//         (wm, wnk, kh) owns the (BM / WGM) x (BN / WGNK) sub-tile over pair kh of every 32-deep chunk (super-steps 2 kh and
//         2 kh + 1: 16 of the chunk's 32 k).  A fragment is then read from LDS and split by ONE wave instead of two.  After the K
//         loop the two waves of a k pair exchange halves of their accumulators through LDS and add: the epilogue sees the layout
//         of WGM x (2 WGNK) waves with wn = 2 wnk + kh (the names WGN, WN, TJ, wn below are the EPILOGUE's; the main loop's are
//         KWN, KTJ, wnk)
//   EMU: 0 = v_mfma_f32_32x32x2_f32; 1 = the same products on the bf16 matrix pipe (split3 above)
template <int BM, int BN, int WGM, int WGNK, int SPEC, int NSTAGE, int WGK = 1, int EMU = 0>
__global__ __launch_bounds__(64 * WGM * WGNK * WGK, 2) void gather_gemm_f32_glds_kernel(const GemmArgs a) {
  static_assert(WGK == 1 || (WGK == 2 && EMU == 1 && SPEC != 2), "K-partitioned waves: two k halves, split-bf16 products, plain operand");
  // Two sets of names.  EPILOGUE layout (everything from the exchange on: gemm_epilogue_rows.inc, gemm_colstats_rows.inc, the
  // staging patches, ecol / ncol): WGN, WN, TJ, wn.  MAIN LOOP (fragment offsets, accumulators, both chunk loops): KWN, KTJ,
  // wnk, kh.  With WGK = 1 the two sets are equal.
  constexpr int WGN = WGNK * WGK;                          // wave columns of the epilogue
  constexpr int NT = 64 * WGM * WGN, NW = NT / 64;
  constexpr int WM = BM / WGM, WN = BN / WGN, KWN = BN / WGNK;
  constexpr int TI = WM / 32, TJ = WN / 32, KTJ = KWN / 32;
  static_assert(TI >= 1 && TJ >= 1 && TI <= 2 && KTJ <= 2 && WM % 32 == 0 && WN % 32 == 0, "wave tile: one to four 32x32 MFMA tiles");
  static_assert(WGK == 1 || (TJ == 1 && KTJ == 2), "K-partitioned waves: the wave keeps one of its two tile columns");
  static_assert(SPEC >= 1 && SPEC <= 3, "SPEC");
  static_assert(NSTAGE >= 2 && NSTAGE <= 4 && (SPEC != 2 || NSTAGE == 2 || NSTAGE == 4), "two to four LDS buffers (two or four with BN on load)");
  constexpr int R = NSTAGE == 4 ? 2 : 1;                   // (xform) register sets = iterations a raw-row load is given
  static_assert(NW % 2 == 0, "the swizzled chunk of a lane is the same for all its rows only with an even wave count");
  static_assert(BN == 64 || BN == 128, "column tiles of 64 or 128");
  constexpr bool xform = SPEC == 2;
  constexpr bool w_nk = SPEC == 3;
  constexpr int BKG = 32;                                  // K chunk in floats: one 128-byte line per row
  constexpr int A_BYTES = BM * 128;
  constexpr int B_ROWB = w_nk ? 128 : BN * 4;              // bytes per row of the weight image
  constexpr int B_BYTES = BN * 128;                        // [BN][32] or [32][BN] floats
  constexpr int STAGE_BYTES = A_BYTES + B_BYTES;
  constexpr int A_INSTR = A_BYTES / (NT * 16), B_INSTR = B_BYTES / (NT * 16);
  static_assert(A_BYTES % (NT * 16) == 0 && B_BYTES % (NT * 16) == 0 && A_INSTR >= 1 && B_INSTR >= 1, "whole 1-KB pieces per wave");
  constexpr int LPS = A_INSTR + B_INSTR;                   // loads per stage (per wave, in vmcnt units)
  constexpr int B_LPR = B_ROWB / 16, B_RPP = 64 / B_LPR;   // lanes per row / rows per 1-KB piece of the weight image

  constexpr int STG_LD = WN + 4;
  constexpr int STG_BYTES = NW * 32 * STG_LD * 4;
  constexpr int TILE_BYTES = NSTAGE * STAGE_BYTES > STG_BYTES ? NSTAGE * STAGE_BYTES : STG_BYTES;
  // one LDS object: [operand stages | epilogue staging][epi: 5 x BN floats][ticket][BN table of the operand (xform)]
  constexpr int OFF_EPI = TILE_BYTES, OFF_TICKET = OFF_EPI + 5 * BN * 4, OFF_BN = OFF_TICKET + 16;
  __shared__ __attribute__((aligned(1024))) unsigned char smem_raw[OFF_BN + (xform ? 2 * MAX_BN_C * 4 : 0)];
  float* const smem = reinterpret_cast<float*>(smem_raw);
  float (*const epi)[BN] = reinterpret_cast<float (*)[BN]>(smem_raw + OFF_EPI);
  int& s_ticket = *reinterpret_cast<int*>(smem_raw + OFF_TICKET);
  float* const bnS = reinterpret_cast<float*>(smem_raw + OFF_BN);
  float* const bnT = bnS + MAX_BN_C;
  bool was_last = false;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WGN, wn = wave % WGN;
  const int wnk = wn / WGK, kh = wn % WGK;                 // main loop: wave column and k half
  unsigned lbx = blockIdx.x, lby = blockIdx.y, lbz = blockIdx.z;
  if (a.xcd_remap) {
    const unsigned inner = gridDim.y * gridDim.z;
    const unsigned sw = xcd_swizzle(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z), gridDim.x * inner);
    lbx = sw / inner;
    const unsigned rem = sw - lbx * inner;
    lby = rem % gridDim.y;
    lbz = rem / gridDim.y;
  }
  const int n0 = lby * BN;
  const int phase = lbz / a.nsplit;
  const int split = lbz - phase * a.nsplit;

  const TapWalk tw = tap_walk(a, phase);
  const int ntx = tw.ntx, ky0 = tw.ky0, kx0 = tw.kx0, kstep_y = tw.kstep_y, kstep_x = tw.kstep_x;
  const int dsgn = tw.dsgn, cy = tw.cy, cx = tw.cx, phy = tw.phy, phx = tw.phx;
  const int nkc = a.Ck / BKG;
  const int total_all = tw.nty * ntx * nkc;
  const __amdgpu_buffer_rsrc_t srdX = __builtin_amdgcn_make_buffer_rsrc((void*)a.X, 0, (int)a.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t srdW = __builtin_amdgcn_make_buffer_rsrc((void*)a.W, 0, (int)a.w_bytes, 0x00020000);
  const int per_split = (total_all + a.nsplit - 1) / a.nsplit;
  const int it_beg = split * per_split;
  const int it_end = it_beg + per_split < total_all ? it_beg + per_split : total_all;
  const int total = it_end > it_beg ? it_end - it_beg : 0;

  const int l31 = lane & 31, lhi = lane >> 5;
  const bool do_relu_bn = a.relu_bn.mode != 0 && !a.mix;
  const int hw = a.Hq * a.Wq;

  if (xform) {
    for (int c = tid; c < a.Ck; c += NT) {
      const BnC k = bn_coef(a.bn_in, c);
      bnS[c] = k.scale;
      bnT[c] = k.shift;
    }
  }
  for (int c = tid; c < BN; c += NT) {
    const int n = n0 + c;
    BnC k = BnC{0.f, 0.f, 0.f, 0.f};
    if (n < a.Cn && (do_relu_bn || a.mix)) k = bn_coef(a.relu_bn, n);
    if (a.mix) { k.scale *= a.mix_a; k.shift *= a.mix_a; }
    epi[0][c] = k.mean; epi[1][c] = k.rstd; epi[2][c] = k.scale; epi[3][c] = k.shift;
    epi[4][c] = (n < a.Cn && a.bias) ? a.bias[n] : 0.f;
  }
  __syncthreads();
  // (epilogue names from here to the fragment offsets)
  constexpr int E_LPR = WN / 8, E_RPP = 64 / E_LPR, E_NPASS = 32 / E_RPP;
  const int c8 = lane % E_LPR, rsub = lane / E_LPR;
  const int ecol = wn * WN + c8 * 8;
  const int ncol = n0 + ecol;
  const bool ok_lo = ncol < a.Cn, ok_hi = ncol + 4 < a.Cn;
  float s1[8], s2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s1[e] = s2[e] = 0.f;
  float* const stg = smem + wave * 32 * STG_LD;
  const unsigned lds_base = (unsigned)(uintptr_t)((lds_void_t*)smem_raw);

  // ---- LDS-DMA source offsets of the weight image ---------------------------------------------------------------------
  unsigned voffB[B_INSTR];
#pragma unroll
  for (int i = 0; i < B_INSTR; ++i) {
    const int pc = i * NW + wave;
    if (w_nk) {
      const int r = 8 * pc + (lane >> 3);
      const int cq = (lane & 7) ^ ((r >> 1) & 7);
      const int n = n0 + r;
      voffB[i] = n < a.Cn ? ((unsigned)n * (unsigned)a.Cout_w + (unsigned)cq * 4u) * 4u : OOB;
    } else {
      const int k = B_RPP * pc + lane / B_LPR;
      const int n = n0 + (lane % B_LPR) * 4;
      voffB[i] = n < a.Cn ? ((unsigned)k * (unsigned)a.Cout_w + (unsigned)n) * 4u : OOB;
    }
  }
  // ---- fragment read offsets (bytes from the stage base; main-loop names: KWN, KTJ, wnk, kh) ---------------------------
  // K-contiguous fragment of super-step q: the lane's row, logical chunk 2 q + lhi
  // (K-partitioned: entry q = 0, 1 is super-step 2 kh + q, the wave's own pair)
  constexpr int NQ = 4 / WGK;
  const int q0 = (WGK - 1) * 2 * kh;
  unsigned aoff[TI][NQ];
#pragma unroll
  for (int i = 0; i < TI; ++i) {
    const int r = wm * WM + i * 32 + l31;
#pragma unroll
    for (int q = 0; q < NQ; ++q) aoff[i][q] = (unsigned)r * 128u + (unsigned)(((2 * (q0 + q) + lhi) ^ ((r >> 1) & 7)) * 16);
  }
  unsigned boff[KTJ][w_nk ? NQ : 1];
#pragma unroll
  for (int j = 0; j < KTJ; ++j) {
    // K-partitioned: the wave's tile column j is column j ^ kh of the block, so that the column a wave KEEPS after the exchange
    // (kh, the epilogue's wn) is acc[.][0] in every wave: a different address, not a different register
    const int jc = WGK == 2 ? (j ^ kh) : j;
    if (w_nk) {
      const int r = wnk * KWN + jc * 32 + l31;
#pragma unroll
      for (int q = 0; q < (w_nk ? NQ : 1); ++q)
        boff[j][q] = (unsigned)A_BYTES + (unsigned)r * 128u + (unsigned)(((2 * (q0 + q) + lhi) ^ ((r >> 1) & 7)) * 16);
    } else {
      // K-strided: k row 8 q + 4 lhi + e (immediate offset (8 q + e) * B_ROWB), column of the lane
      boff[j][0] = (unsigned)A_BYTES + (unsigned)(8 * q0 + 4 * lhi) * (unsigned)B_ROWB + (unsigned)(wnk * KWN + jc * 32 + l31) * 4u;
    }
  }

  const long nMt = (a.rows_per_phase + BM - 1) / BM;
  for (long mt = lbx; mt < nMt; mt += gridDim.x) {
    const long m0 = mt * BM;

    int ry0[A_INSTR], rx0[A_INSTR], rbase[A_INSTR];
    unsigned cqA[A_INSTR];
    bool rvalid[A_INSTR];
#pragma unroll
    for (int i = 0; i < A_INSTR; ++i) {
      const int r = 8 * (i * NW + wave) + (lane >> 3);
      cqA[i] = (unsigned)(((lane & 7) ^ ((r >> 1) & 7)) * 16);
      const long m = m0 + r;
      rvalid[i] = m < a.rows_per_phase;
      const unsigned mm = rvalid[i] ? (unsigned)m : 0u;
      const int n = (int)(mm / (unsigned)hw);
      const int rem = (int)(mm - (unsigned)n * (unsigned)hw);
      const int qy = rem / a.Wq, qx = rem - qy * a.Wq;
      if (a.form == 0) { ry0[i] = qy * a.sh - a.ph; rx0[i] = qx * a.sw - a.pw; }
      else             { ry0[i] = qy + cy;          rx0[i] = qx + cx; }
      rbase[i] = (n * a.Hx + ry0[i]) * a.Wx + rx0[i];
    }

    int ld_tap = it_beg / nkc;
    int ld_kc = (it_beg - ld_tap * nkc) * BKG;
    bool tap_dirty = true;
    unsigned offA[A_INSTR], offW = 0;

    float4 ra[xform ? R : 1][xform ? A_INSTR : 1];
    bool pend_ok[xform ? R : 1][xform ? A_INSTR : 1];
    float4 psc[xform ? R : 1], psh[xform ? R : 1];
    unsigned sB_set[xform ? R : 1];
    bool okA[A_INSTR];
    // plain: one stage = LPS LDS-DMA instructions into buffer `buf`.  xform: the stage's raw rows into register set `buf`
    // (with the row-valid flags, the BatchNorm coefficients of this lane's four channels and the weights' scalar offset)
    auto issue = [&](auto bufc) {
      constexpr int buf = decltype(bufc)::value;
      if (tap_dirty) {
        const int jy = ld_tap / ntx, jx = ld_tap - jy * ntx;
        const int wtap = (ky0 + kstep_y * jy) * a.kw + (kx0 + kstep_x * jx);
        const int tapoff = dsgn * (jy * a.Wx + jx);
#pragma unroll
        for (int i = 0; i < A_INSTR; ++i) {
          const int iy = ry0[i] + dsgn * jy, ix = rx0[i] + dsgn * jx;
          const bool ok = rvalid[i] & ((unsigned)iy < (unsigned)a.Hx) & ((unsigned)ix < (unsigned)a.Wx);
          offA[i] = ok ? (unsigned)(rbase[i] + tapoff) * (unsigned)a.Ck * 4u + cqA[i] : OOB;
          okA[i] = ok;
        }
        offW = (unsigned)wtap * (unsigned)a.Cin_w * (unsigned)a.Cout_w * 4u;
        tap_dirty = false;
      }
      const unsigned sA = (unsigned)ld_kc * 4u;
      const unsigned sB = offW + (w_nk ? (unsigned)ld_kc * 4u : (unsigned)ld_kc * (unsigned)a.Cout_w * 4u);
      if constexpr (xform) {
        constexpr int set = buf;
        const int kch = ld_kc + (int)(cqA[0] >> 2);          // first of this lane's four channels (the same for all its rows)
        {   // (read in assembly, like the fragments: an LDS read the compiler can see waits for every LDS-DMA in flight)
          u32x4 cs, ct;
          lds_load_coef2(cs, ct, lds_base + (unsigned)OFF_BN + (unsigned)kch * 4u, lds_base + (unsigned)OFF_BN + (unsigned)(MAX_BN_C + kch) * 4u);
          psc[set] = __builtin_bit_cast(float4, cs);
          psh[set] = __builtin_bit_cast(float4, ct);
        }
#pragma unroll
        for (int i = 0; i < A_INSTR; ++i) { ra[set][i] = bld4s(srdX, offA[i], sA); pend_ok[set][i] = okA[i]; }
        sB_set[set] = sB;
      } else {
        unsigned char* const stage = smem_raw + buf * STAGE_BYTES;
#pragma unroll
        for (int i = 0; i < A_INSTR; ++i) lds_dma16(srdX, stage + (i * NW + wave) * 1024, offA[i], sA);
#pragma unroll
        for (int i = 0; i < B_INSTR; ++i) lds_dma16(srdW, stage + A_BYTES + (i * NW + wave) * 1024, voffB[i], sB);
      }
      ld_kc += BKG;
      if (ld_kc >= a.Ck) { ld_kc = 0; ++ld_tap; tap_dirty = true; }
    };
    // xform: register set `set` -> BN, ReLU -> the LDS image of buffer `buf`; then that stage's weights by DMA (issued AFTER
    // the ds_writes, so nothing is in flight into LDS while they are emitted)
    auto commit = [&](auto bufc, auto setc) {
      constexpr int buf = decltype(bufc)::value, set = xform ? decltype(setc)::value : 0;
      unsigned char* const stage = smem_raw + buf * STAGE_BYTES;
#pragma unroll
      for (int i = 0; i < A_INSTR; ++i) {
        const float4 v = ra[set][xform ? i : 0];
        float4 t;
        t.x = fmaxf(fmaf(v.x, psc[set].x, psh[set].x), 0.f); t.y = fmaxf(fmaf(v.y, psc[set].y, psh[set].y), 0.f);
        t.z = fmaxf(fmaf(v.z, psc[set].z, psh[set].z), 0.f); t.w = fmaxf(fmaf(v.w, psc[set].w, psh[set].w), 0.f);
        if (!pend_ok[set][xform ? i : 0]) t = make_float4(0.f, 0.f, 0.f, 0.f);     // spatial padding stays zero AFTER the transform
        // (the store in assembly: one the compiler can see waits for every LDS-DMA in flight -- it had moved the weights' DMA of
        // this commit in front of the stores and put `s_waitcnt vmcnt(0)` before the first of them)
        lds_store_b128(lds_base + (unsigned)(buf * STAGE_BYTES + (i * NW + wave) * 1024) + (unsigned)lane * 16u, __builtin_bit_cast(u32x4, t));
      }
#pragma unroll
      for (int i = 0; i < B_INSTR; ++i) lds_dma16(srdW, stage + A_BYTES + (i * NW + wave) * 1024, voffB[i], sB_set[set]);
    };

    f32x16 acc[TI][KTJ];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int j = 0; j < KTJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // prologue: stages 0 .. NSTAGE-2 in flight.  xform: raw rows of stages 0 .. R-1 requested, then stage c = 0 .. NSTAGE-2
    // committed to buffer c from set c % R, each followed by the request for stage c + R into the set it freed
    using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>; using I3 = std::integral_constant<int, 3>;
    if constexpr (xform) {
      if (total > 0) issue(I0{});
      if constexpr (R == 2) { if (total > 1) issue(I1{}); }
      if (total > 0) commit(I0{}, I0{});
      if (total > R) issue(I0{});
      if constexpr (NSTAGE == 4) {
        if (total > 1) commit(I1{}, I1{});
        if (total > 1 + R) issue(I1{});
        if (total > 2) commit(I2{}, I0{});
        if (total > 2 + R) issue(I0{});
      }
    } else {
      if (total > 0) issue(I0{});
      if (NSTAGE >= 3 && total > 1) issue(I1{});
      if (NSTAGE >= 4 && total > 2) issue(I2{});
    }

    auto chunk = [&](int it, auto curc) {
      constexpr int cur = decltype(curc)::value;
      if constexpr (xform) {
        // needed now: the weights of stage `it` (DMA) and the raw rows of stage c = it + NSTAGE - 1 (requested R iterations
        // ago).  Younger than both: the (R - 1) x (weights DMA + raw-row loads) of the iterations in between -- if all of
        // them were issued (not at the tail of the tile: then wait for everything)
        if (R == 2 && it + NSTAGE - 2 + R < total) wait_vmcnt<LPS>();
        else wait_vmcnt<0>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's ds_writes of earlier commits
      } else {
        // this wave's DMAs of stage `it` have landed when at most min(NSTAGE - 2, stages left behind it) younger stages are out
        const int younger = total - 1 - it < NSTAGE - 2 ? total - 1 - it : NSTAGE - 2;
        if (NSTAGE >= 4 && younger == 2) wait_vmcnt<2 * LPS>();
        else if (NSTAGE >= 3 && younger == 1) wait_vmcnt<LPS>();
        else wait_vmcnt<0>();
      }
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (xform) {
        constexpr int cbuf = (cur + NSTAGE - 1) % NSTAGE, cset = (cur + NSTAGE - 1) % R;
        if (it + NSTAGE - 1 < total) commit(std::integral_constant<int, cbuf>{}, std::integral_constant<int, cset>{});
        if (it + NSTAGE - 1 + R < total) issue(std::integral_constant<int, cset>{});
        __builtin_amdgcn_sched_barrier(0);
      } else {
        if (it + NSTAGE - 1 < total) issue(std::integral_constant<int, (cur + NSTAGE - 1) % NSTAGE>{});
      }
      constexpr unsigned stage_off = (unsigned)(cur * STAGE_BYTES);
      f32x4v fa[2][TI], fb[2][w_nk ? KTJ : 1];
      float fk[2][w_nk ? 1 : KTJ][4];
      auto read_step = [&](auto qc, auto setc) {
        constexpr int q = decltype(qc)::value, set = decltype(setc)::value;
#pragma unroll
        for (int i = 0; i < TI; ++i) lds_frag_f4<0>(fa[set][i], lds_base + stage_off + aoff[i][q]);
        if constexpr (w_nk) {
#pragma unroll
          for (int j = 0; j < KTJ; ++j) lds_frag_f4<0>(fb[set][j], lds_base + stage_off + boff[j][w_nk ? q : 0]);
        } else {
#pragma unroll
          for (int j = 0; j < KTJ; ++j) {
            lds_frag_f1<(8 * q + 0) * B_ROWB>(fk[set][j][0], lds_base + stage_off + boff[j][0]);
            lds_frag_f1<(8 * q + 1) * B_ROWB>(fk[set][j][1], lds_base + stage_off + boff[j][0]);
            lds_frag_f1<(8 * q + 2) * B_ROWB>(fk[set][j][2], lds_base + stage_off + boff[j][0]);
            lds_frag_f1<(8 * q + 3) * B_ROWB>(fk[set][j][3], lds_base + stage_off + boff[j][0]);
          }
        }
      };
      auto fence = [&](auto setc) {
        constexpr int set = decltype(setc)::value;
        if constexpr (w_nk) {
          if constexpr (TI == 2 && KTJ == 2) MOPOE_DEVICE_ASM("s_waitcnt lgkmcnt(0)" : "+v"(fa[set][0]), "+v"(fa[set][1]), "+v"(fb[set][0]), "+v"(fb[set][1]) :: "memory");
          else if constexpr (TI == 2) MOPOE_DEVICE_ASM("s_waitcnt lgkmcnt(0)" : "+v"(fa[set][0]), "+v"(fa[set][1]), "+v"(fb[set][0]) :: "memory");
          else if constexpr (KTJ == 2) MOPOE_DEVICE_ASM("s_waitcnt lgkmcnt(0)" : "+v"(fa[set][0]), "+v"(fb[set][0]), "+v"(fb[set][1]) :: "memory");
          else MOPOE_DEVICE_ASM("s_waitcnt lgkmcnt(0)" : "+v"(fa[set][0]), "+v"(fb[set][0]) :: "memory");
        } else {
          if constexpr (TI == 2 && KTJ == 2)
            MOPOE_DEVICE_ASM("s_waitcnt lgkmcnt(0)" : "+v"(fa[set][0]), "+v"(fa[set][1]), "+v"(fk[set][0][0]), "+v"(fk[set][0][1]), "+v"(fk[set][0][2]),
                             "+v"(fk[set][0][3]), "+v"(fk[set][1][0]), "+v"(fk[set][1][1]), "+v"(fk[set][1][2]), "+v"(fk[set][1][3]) :: "memory");
          else if constexpr (TI == 2)
            MOPOE_DEVICE_ASM("s_waitcnt lgkmcnt(0)" : "+v"(fa[set][0]), "+v"(fa[set][1]), "+v"(fk[set][0][0]), "+v"(fk[set][0][1]), "+v"(fk[set][0][2]),
                             "+v"(fk[set][0][3]) :: "memory");
          else if constexpr (KTJ == 2)
            MOPOE_DEVICE_ASM("s_waitcnt lgkmcnt(0)" : "+v"(fa[set][0]), "+v"(fk[set][0][0]), "+v"(fk[set][0][1]), "+v"(fk[set][0][2]),
                             "+v"(fk[set][0][3]), "+v"(fk[set][1][0]), "+v"(fk[set][1][1]), "+v"(fk[set][1][2]), "+v"(fk[set][1][3]) :: "memory");
          else
            MOPOE_DEVICE_ASM("s_waitcnt lgkmcnt(0)" : "+v"(fa[set][0]), "+v"(fk[set][0][0]), "+v"(fk[set][0][1]), "+v"(fk[set][0][2]),
                             "+v"(fk[set][0][3]) :: "memory");
        }
        __builtin_amdgcn_sched_barrier(0);
      };
      auto mfma_step = [&](auto setc) {
        constexpr int set = decltype(setc)::value;
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int j = 0; j < KTJ; ++j) {
            const float b = w_nk ? fb[set][w_nk ? j : 0][e] : fk[set][w_nk ? 0 : j][e];
#pragma unroll
            for (int i = 0; i < TI; ++i)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set][i][e], b, acc[i][j], 0, 0, 0);
          }
      };
      using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>;
      using I2 = std::integral_constant<int, 2>; using I3 = std::integral_constant<int, 3>;
      read_step(I0{}, I0{});
      fence(I0{});
      read_step(I1{}, I1{});
      mfma_step(I0{});
      fence(I1{});
      read_step(I2{}, I0{});
      mfma_step(I1{});
      fence(I0{});
      read_step(I3{}, I1{});
      mfma_step(I0{});
      fence(I1{});
      mfma_step(I1{});
      __builtin_amdgcn_sched_barrier(0);
    };
    if constexpr (EMU != 0) {
#include "conv_gemm_glds_emu.inc"
    } else {
      int it = 0;
      while (it < total) {
        chunk(it, std::integral_constant<int, 0>{});
        if (++it >= total) break;
        chunk(it, std::integral_constant<int, 1>{});
        if (++it >= total) break;
        if (NSTAGE >= 3) {
          chunk(it, std::integral_constant<int, 2 % NSTAGE>{});
          if (++it >= total) break;
        }
        if (NSTAGE >= 4) {
          chunk(it, std::integral_constant<int, 3 % NSTAGE>{});
          ++it;
        }
      }
    }
    __syncthreads();   // every wave is done with the operand buffers: the epilogue's staging patches overlay them

    if constexpr (WGK == 2) {
      // ---- K-partitioned waves: one reduction across the two k halves per M tile -----------------------------------
      // Wave (wm, kh) keeps tile column kh of the block -- its acc[.][0], see boff -- and gets the partner's sums for it; the other
      // column, acc[.][1], goes to the partner (wave ^ 1) through a private TI x 4 KB slot at the start of the operand stages.
      // Those are dead: the last chunk's top waited for vmcnt(0) in every wave (no LDS-DMA of this tile is in flight), and the
      // barrier above says both k halves have read their fragments of it.  The next tile's prologue DMA is issued behind the
      // barrier that ends the epilogue.  The accesses are assembly, like every LDS access of the main loop; the wave counts
      // lgkmcnt for them itself.  Only the order of fp32 additions differs from one wave walking all of k: two chains over half
      // the k each, then one add.
      constexpr int X_BYTES = TI * 4096;
      static_assert(NW * X_BYTES <= NSTAGE * STAGE_BYTES, "the exchange slots overlay the operand stages");
      const unsigned x_own = lds_base + (unsigned)(wave * X_BYTES) + (unsigned)lane * 16u;
      const unsigned x_partner = lds_base + (unsigned)((wave ^ 1) * X_BYTES) + (unsigned)lane * 16u;
      // (plain loops: a lambda that is not inlined here would put the accumulators into scratch memory)
#pragma unroll
      for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          lds_store_b128(x_own + (unsigned)((i * 4 + g) * 1024),
                         u32x4{__float_as_uint(acc[i][1][4 * g]), __float_as_uint(acc[i][1][4 * g + 1]), __float_as_uint(acc[i][1][4 * g + 2]),
                               __float_as_uint(acc[i][1][4 * g + 3])});
      MOPOE_DEVICE_ASM("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 0; i < TI; ++i) {
        u32x4 t0, t1, t2, t3;
        lds_load_x4(t0, t1, t2, t3, x_partner + (unsigned)(i * 4096));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc[i][0][e] += __uint_as_float(t0[e]);
          acc[i][0][4 + e] += __uint_as_float(t1[e]);
          acc[i][0][8 + e] += __uint_as_float(t2[e]);
          acc[i][0][12 + e] += __uint_as_float(t3[e]);
        }
      }
      __syncthreads();   // every wave has read its partner's slot: the staging patches overlay the slots too
    }

    // (epilogue names from here on: acc[i][j], j < TJ)
#include "gemm_epilogue_rows.inc"
  }

#include "gemm_colstats_rows.inc"
}

// =====================================================================================================
// Weight gradient (fp32) on LDS-DMA: dWp[tap][ci][co] = sum over pixels of T(x)[pixel][ci] * dy[pixel][co].
// Both operands are K-strided ([pixel][channel] rows as they lie in memory, 32 pixels per stage), so both fragments are read
// like the forward weights above: one ds_read_b32 per MFMA and operand, 32 consecutive lanes = 32 consecutive channels of
// one pixel row (no bank conflicts, no permutation).  The gradient rows always arrive by DMA; the activation rows too unless
// BN -> ReLU is applied to them (XFORM: through registers, two buffers).  Grid, split of the pixel reduction and the
// atomic accumulation are those of wgrad_gemm_kernel.
// =====================================================================================================
//   EMU: 0 = v_mfma_f32_32x32x2_f32; 1 = the same products on the bf16 matrix pipe (split3 above; plain operands only)
template <int BI, bool XFORM, int NSTAGE, int EMU = 0>
__global__ __launch_bounds__(256, 2) void wgrad_gemm_f32_glds_kernel(const WgradArgs a) {
  static_assert(EMU == 0 || !XFORM, "EMU: plain operand form");
  constexpr int BJ = BI;
  constexpr int WI = BI / 2, WJ = BJ / 2, TI = WI / 32, TJ = WJ / 32;
  constexpr int KP = 32;                                   // pixels per stage
  constexpr int ROWB = BI * 4;                             // bytes per pixel row of either image
  static_assert(BI == 64 || BI == 128, "tiles of 64 or 128 channels");
  static_assert(NSTAGE >= 2 && NSTAGE <= 4 && (!XFORM || NSTAGE == 2), "two to four LDS buffers (two with BN on load)");
  constexpr int LPR = ROWB / 16, RPP = 64 / LPR;           // lanes per row, rows per 1-KB piece
  constexpr int IMG_BYTES = KP * ROWB;
  constexpr int STAGE_BYTES = 2 * IMG_BYTES;
  constexpr int NINSTR = IMG_BYTES / (256 * 16);           // DMA instructions per thread, stage and operand
  static_assert(IMG_BYTES % (256 * 16) == 0 && NINSTR >= 1, "whole pieces");
  constexpr int LPS = 2 * NINSTR;
  constexpr int OFF_BN = NSTAGE * STAGE_BYTES;
  __shared__ __attribute__((aligned(1024))) unsigned char smem[OFF_BN + (XFORM ? 2 * MAX_BN_C * 4 : 16)];
  float* const bnS = reinterpret_cast<float*>(smem + OFF_BN);
  float* const bnT = bnS + MAX_BN_C;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wi = wave >> 1, wj = wave & 1;
  const unsigned lin = a.xcd_remap ? xcd_swizzle(blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z),
                                                 gridDim.x * gridDim.y * gridDim.z)
                                   : blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  const unsigned bx = lin % gridDim.x, byz = lin / gridDim.x;
  const unsigned by = byz % gridDim.y, bz = byz / gridDim.y;
  const int it_i = bx / a.nJ, it_j = bx % a.nJ;
  const int i0 = it_i * BI, j0 = it_j * BJ;
  const int tap = by;
  const int ky = tap / a.kw, kx = tap % a.kw;
  const long mbeg = (long)bz * a.chunk;
  const long mend = mbeg + a.chunk < a.Ms ? mbeg + a.chunk : a.Ms;
  const int total = (int)((mend - mbeg + KP - 1) / KP);

  if (XFORM) {
    for (int c = tid; c < ((a.Cin + 3) & ~3); c += 256) {
      BnC k = BnC{0.f, 0.f, 0.f, 0.f};
      if (c < a.Cin) k = bn_coef(a.bn_in, c);
      bnS[c] = k.scale;
      bnT[c] = k.shift;
    }
    __syncthreads();
  }
  const __amdgpu_buffer_rsrc_t srdX = __builtin_amdgcn_make_buffer_rsrc((void*)a.Xs, 0, (int)a.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t srdD = __builtin_amdgcn_make_buffer_rsrc((void*)a.Dy, 0, (int)a.dy_bytes, 0x00020000);
  const unsigned lds_base = (unsigned)(uintptr_t)((lds_void_t*)smem);

  // this lane's slot in every 1-KB piece: pixel slot RPP * piece + lane / LPR, channels 4 (lane % LPR) .. + 3 of the tile
  const int slot_in_piece = lane / LPR;
  const int ci = i0 + (lane % LPR) * 4, cj = j0 + (lane % LPR) * 4;
  const bool ci_ok = ci < a.Cin, cj_ok = cj < a.Cout;     // (Cin, Cout % 4 == 0 on the vector path: the four channels go together)
  float4 sc = make_float4(0.f, 0.f, 0.f, 0.f), sh = sc;
  if (XFORM && ci_ok) {
    sc = *reinterpret_cast<const float4*>(&bnS[ci]);
    sh = *reinterpret_cast<const float4*>(&bnT[ci]);
  }
  const unsigned hw = (unsigned)(a.Hs * a.Ws);

  // fragment read offsets: pixel row 8 q + 4 lhi + e (immediate offset (8 q + e) * ROWB), channel of the lane
  unsigned ioff[TI], joff[TJ];
  {
    const int l31 = lane & 31, lhi = lane >> 5;
#pragma unroll
    for (int i = 0; i < TI; ++i) ioff[i] = (unsigned)(4 * lhi) * (unsigned)ROWB + (unsigned)(wi * WI + i * 32 + l31) * 4u;
#pragma unroll
    for (int j = 0; j < TJ; ++j) joff[j] = (unsigned)IMG_BYTES + (unsigned)(4 * lhi) * (unsigned)ROWB + (unsigned)(wj * WJ + j * 32 + l31) * 4u;
  }

  float4 ri[XFORM ? NINSTR : 1];
  bool okx_reg[XFORM ? NINSTR : 1];
  unsigned offd_pending[XFORM ? NINSTR : 1];
  unsigned m_next = (unsigned)mbeg;

  auto offsets = [&](unsigned (&offx)[NINSTR], unsigned (&offd)[NINSTR], bool (&okx)[NINSTR]) {
#pragma unroll
    for (int t = 0; t < NINSTR; ++t) {
      const unsigned m = m_next + (unsigned)(RPP * (t * 4 + wave) + slot_in_piece);
      const bool inm = (long)m < mend;
      const unsigned n = m / hw;
      const unsigned rem = m - n * hw;
      const unsigned qy = rem / (unsigned)a.Ws, qx = rem - qy * (unsigned)a.Ws;
      const int yb = (int)qy * a.sh - a.ph + ky, xb = (int)qx * a.sw - a.pw + kx;
      const bool inb = ((unsigned)yb < (unsigned)a.Hb) & ((unsigned)xb < (unsigned)a.Wb);
      const unsigned brow = (n * (unsigned)a.Hb + (unsigned)yb) * (unsigned)a.Wb + (unsigned)xb;
      const unsigned rowx = a.x_is_big ? brow : m, rowd = a.x_is_big ? m : brow;
      okx[t] = inm & ci_ok & (a.x_is_big ? inb : true);
      const bool okd = inm & cj_ok & (a.x_is_big ? true : inb);
      offx[t] = okx[t] ? (rowx * (unsigned)a.Cin + (unsigned)ci) * 4u : OOB;
      offd[t] = okd ? (rowd * (unsigned)a.Cout + (unsigned)cj) * 4u : OOB;
    }
    m_next += KP;
  };
  auto issue = [&](auto bufc) {
    constexpr int buf = decltype(bufc)::value;
    unsigned offx[NINSTR], offd[NINSTR];
    bool okx[NINSTR];
    offsets(offx, offd, okx);
    unsigned char* const stage = smem + buf * STAGE_BYTES;
    if constexpr (XFORM) {
#pragma unroll
      for (int t = 0; t < NINSTR; ++t) { ri[t] = bld4(srdX, offx[t]); okx_reg[t] = okx[t]; offd_pending[t] = offd[t]; }
    } else {
#pragma unroll
      for (int t = 0; t < NINSTR; ++t) lds_dma16(srdX, stage + (t * 4 + wave) * 1024, offx[t], 0u);
#pragma unroll
      for (int t = 0; t < NINSTR; ++t) lds_dma16(srdD, stage + IMG_BYTES + (t * 4 + wave) * 1024, offd[t], 0u);
    }
  };
  auto commit = [&](auto bufc) {
    constexpr int buf = decltype(bufc)::value;
    unsigned char* const stage = smem + buf * STAGE_BYTES;
#pragma unroll
    for (int t = 0; t < NINSTR; ++t) {
      const float4 v = ri[XFORM ? t : 0];
      float4 o;
      o.x = fmaxf(fmaf(v.x, sc.x, sh.x), 0.f); o.y = fmaxf(fmaf(v.y, sc.y, sh.y), 0.f);
      o.z = fmaxf(fmaf(v.z, sc.z, sh.z), 0.f); o.w = fmaxf(fmaf(v.w, sc.w, sh.w), 0.f);
      if (!okx_reg[XFORM ? t : 0]) o = make_float4(0.f, 0.f, 0.f, 0.f);
      lds_store_b128(lds_base + (unsigned)(buf * STAGE_BYTES + (t * 4 + wave) * 1024) + (unsigned)lane * 16u, __builtin_bit_cast(u32x4, o));
    }
#pragma unroll
    for (int t = 0; t < NINSTR; ++t) lds_dma16(srdD, stage + IMG_BYTES + (t * 4 + wave) * 1024, offd_pending[XFORM ? t : 0], 0u);
  };

  f32x16 acc[TI][TJ];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < TJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  if (total > 0) issue(std::integral_constant<int, 0>{});
  if constexpr (XFORM) {
    if (total > 0) commit(std::integral_constant<int, 0>{});
    if (total > 1) issue(std::integral_constant<int, 1>{});
  } else {
    if (NSTAGE >= 3 && total > 1) issue(std::integral_constant<int, 1>{});
    if (NSTAGE >= 4 && total > 2) issue(std::integral_constant<int, 2>{});
  }

  auto chunk = [&](int it, auto curc) {
    constexpr int cur = decltype(curc)::value;
    const int younger = total - 1 - it < NSTAGE - 2 ? total - 1 - it : NSTAGE - 2;
    if (NSTAGE >= 4 && younger == 2) wait_vmcnt<2 * LPS>();
    else if (NSTAGE >= 3 && younger == 1) wait_vmcnt<LPS>();
    else wait_vmcnt<0>();
    if constexpr (XFORM) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (XFORM) {
      if (it + 1 < total) commit(std::integral_constant<int, cur ^ 1>{});
      if (it + 2 < total) issue(std::integral_constant<int, cur>{});
      __builtin_amdgcn_sched_barrier(0);
    } else {
      if (it + NSTAGE - 1 < total) issue(std::integral_constant<int, (cur + NSTAGE - 1) % NSTAGE>{});
    }
    constexpr unsigned stage_off = (unsigned)(cur * STAGE_BYTES);
    float fa[2][TI][4], fb[2][TJ][4];
    auto read_step = [&](auto qc, auto setc) {
      constexpr int q = decltype(qc)::value, set = decltype(setc)::value;
#pragma unroll
      for (int i = 0; i < TI; ++i) {
        lds_frag_f1<(8 * q + 0) * ROWB>(fa[set][i][0], lds_base + stage_off + ioff[i]);
        lds_frag_f1<(8 * q + 1) * ROWB>(fa[set][i][1], lds_base + stage_off + ioff[i]);
        lds_frag_f1<(8 * q + 2) * ROWB>(fa[set][i][2], lds_base + stage_off + ioff[i]);
        lds_frag_f1<(8 * q + 3) * ROWB>(fa[set][i][3], lds_base + stage_off + ioff[i]);
      }
#pragma unroll
      for (int j = 0; j < TJ; ++j) {
        lds_frag_f1<(8 * q + 0) * ROWB>(fb[set][j][0], lds_base + stage_off + joff[j]);
        lds_frag_f1<(8 * q + 1) * ROWB>(fb[set][j][1], lds_base + stage_off + joff[j]);
        lds_frag_f1<(8 * q + 2) * ROWB>(fb[set][j][2], lds_base + stage_off + joff[j]);
        lds_frag_f1<(8 * q + 3) * ROWB>(fb[set][j][3], lds_base + stage_off + joff[j]);
      }
    };
    auto fence = [&](auto setc) {
      constexpr int set = decltype(setc)::value;
      if constexpr (TI == 2)
        MOPOE_DEVICE_ASM("s_waitcnt lgkmcnt(0)" : "+v"(fa[set][0][0]), "+v"(fa[set][0][1]), "+v"(fa[set][0][2]), "+v"(fa[set][0][3]),
                         "+v"(fa[set][1][0]), "+v"(fa[set][1][1]), "+v"(fa[set][1][2]), "+v"(fa[set][1][3]),
                         "+v"(fb[set][0][0]), "+v"(fb[set][0][1]), "+v"(fb[set][0][2]), "+v"(fb[set][0][3]),
                         "+v"(fb[set][1][0]), "+v"(fb[set][1][1]), "+v"(fb[set][1][2]), "+v"(fb[set][1][3]) :: "memory");
      else
        MOPOE_DEVICE_ASM("s_waitcnt lgkmcnt(0)" : "+v"(fa[set][0][0]), "+v"(fa[set][0][1]), "+v"(fa[set][0][2]), "+v"(fa[set][0][3]),
                         "+v"(fb[set][0][0]), "+v"(fb[set][0][1]), "+v"(fb[set][0][2]), "+v"(fb[set][0][3]) :: "memory");
      __builtin_amdgcn_sched_barrier(0);
    };
    auto mfma_step = [&](auto setc) {
      constexpr int set = decltype(setc)::value;
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
#pragma unroll
          for (int i = 0; i < TI; ++i)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set][i][e], fb[set][j][e], acc[i][j], 0, 0, 0);
    };
    using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>; using I3 = std::integral_constant<int, 3>;
    if constexpr (EMU != 0) {
      // two pairs of super-steps = two bf16 MFMA steps of 16 pixels (conv_gemm_glds_emu.inc: the same phases)
      Split3 sa[2][TI], sb[2][TJ];
      auto fence_both = [&]() {
        MOPOE_DEVICE_ASM("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int i = 0; i < TI; ++i) pin_reg(fa[s][i][e]);
#pragma unroll
            for (int j = 0; j < TJ; ++j) pin_reg(fb[s][j][e]);
          }
        __builtin_amdgcn_sched_barrier(0);
      };
      auto split_pair = [&](auto pc) {
        constexpr int p = decltype(pc)::value;
#pragma unroll
        for (int i = 0; i < TI; ++i) sa[p][i] = split3(fa[0][i], fa[1][i]);
#pragma unroll
        for (int j = 0; j < TJ; ++j) sb[p][j] = split3(fb[0][j], fb[1][j]);
      };
      auto mfma_pair = [&](auto pc) {
        constexpr int p = decltype(pc)::value;
        static_for<6>([&](auto tc) {
#pragma unroll
          for (int j = 0; j < TJ; ++j)
#pragma unroll
            for (int i = 0; i < TI; ++i) mfma_split_term<decltype(tc)::value>(acc[i][j], sa[p][i], sb[p][j]);
        });
      };
      read_step(I0{}, I0{});
      read_step(I1{}, I1{});
      fence_both();
      split_pair(I0{});
      __builtin_amdgcn_sched_barrier(0);
      read_step(I2{}, I0{});
      read_step(I3{}, I1{});
      mfma_pair(I0{});
      __builtin_amdgcn_sched_barrier(0);
      fence_both();
      split_pair(I1{});
      __builtin_amdgcn_sched_barrier(0);
      mfma_pair(I1{});
      __builtin_amdgcn_sched_barrier(0);
    } else {
    read_step(I0{}, I0{});
    fence(I0{});
    read_step(I1{}, I1{});
    mfma_step(I0{});
    fence(I1{});
    read_step(I2{}, I0{});
    mfma_step(I1{});
    fence(I0{});
    read_step(I3{}, I1{});
    mfma_step(I0{});
    fence(I1{});
    mfma_step(I1{});
    __builtin_amdgcn_sched_barrier(0);
    }
  };
  {
    int it = 0;
    while (it < total) {
      chunk(it, std::integral_constant<int, 0>{});
      if (++it >= total) break;
      chunk(it, std::integral_constant<int, 1>{});
      if (++it >= total) break;
      if (NSTAGE >= 3) {
        chunk(it, std::integral_constant<int, 2 % NSTAGE>{});
        if (++it >= total) break;
      }
      if (NSTAGE >= 4) {
        chunk(it, std::integral_constant<int, 3 % NSTAGE>{});
        ++it;
      }
    }
  }

  const int l31 = lane & 31, lhi = lane >> 5;
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    const int co = j0 + wj * WJ + j * 32 + l31;
    if (co >= a.Cout) continue;
#pragma unroll
    for (int i = 0; i < TI; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int cii = i0 + wi * WI + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
        if (cii >= a.Cin) continue;
        float* dst = a.dW + ((long)tap * a.Cin + cii) * a.Cout + co;
        if (a.atomic) unsafeAtomicAdd(dst, acc[i][j][r]);
        else *dst = acc[i][j][r];
      }
    }
  }
}
