// Weight-stationary, software-pipelined, persistent FP32-MFMA linear kernel for the big N-row layers (gfx950).
//
// One workgroup per CU, four waves = one per SIMD (each owns all 512 registers of its SIMD), each wave a 64 x 64 block of the
// 64 x 256 output tile (2 x 2 v_mfma_f32_32x32x2_f32 accumulators); the workgroup walks row tiles b, b + grid, ...
//
// WEIGHT-STATIONARY: a wave's 64 columns x K slab of the packed weight image (K = 256: 64 KiB = 256 registers per lane) is
// loaded ONCE per launch, straight into the wave's 256 AGPRs (global_load_dwordx4 with an AGPR destination), and is the B
// operand of every MFMA from there; the accumulators live in VGPRs, so the epilogue needs no v_accvgpr_read.  Nothing but
// activations then moves per tile: the launch's L2 -> CU weight traffic drops from one slab per TILE (512 MB per launch at
// 131072 rows) to one slab per workgroup (64 MB), the K loop carries no weight loads and no vmcnt waits for them.  Why it
// matters: the N-row kernels run power-limited (in-kernel clock 2.07 GHz against 2.38 GHz for bare MFMAs on the same
// device, scratch/mfma/clock.hip), so bytes moved are time twice - as stalls and as clock.
//
// What the design rests on (all measured on MI355X, sources under scratch/mfma/):
//  * dep.hip       155 TFLOP/s from any number of waves per SIMD: one wave with four accumulators saturates the pipe.
//  * ws.hip        the same rate with B operands in AGPRs, accumulators in VGPRs and SrcC = 0 on a tile's first MFMAs.
//  * samewave.hip  FP32 MFMA and the vector ALU are ONE resource: every v_* instruction, from this wave or another,
//                  adds its 4 cycles to the matrix time.  So VALU work is priced, never hidden - keep it minimal.
//  * ldasm.hip     a wave that waits for operand loads right before using them loses 20-40 % whatever the occupancy;
//                  loads must be in flight inside the wave's own MFMA stream.  hipcc does not keep such a schedule (it
//                  sinks prefetches to their use), hence the inline-asm loads, MFMAs and s_waitcnt below.
//
// Each wave runs ONE continuous instruction stream in which every memory access is issued long before its use:
//   * activation fragments: ds_read_b128, one chunk ahead, running across panel and tile boundaries;
//   * activation panels (64 rows x 64 k) HBM -> registers at chunk 0 of the previous panel, -> LDS at chunk NCH-3, one
//     s_barrier at chunk NCH-2; three LDS buffers make the single barrier per panel sufficient;
//   * the previous tile's results (1-2 tensors, kept in place in the operand registers) are stored behind the MFMAs of the
//     first chunks of the tile, the epilogue's saved-activation operands (S, R / Q, sigma) are loaded into the SAME registers
//     behind the MFMAs of the following chunks, the last one >= 5 chunks (2 us) before the epilogue needs it.
// vmcnt retires in order, so the one wait inside the K loop (panel registers -> LDS) is a compile-time count (Sched).
// MFMAs are inline asm too (AGPR operands), so the hazard recogniser does not see them: the explicit s_nop after a tile's
// last MFMA covers the wait states before the vector ALU may read its result.
//
// Shapes: M % 64 == 0, Nout % 256 == 0, ONE source with K = 256 or 32 (the slab must fit the AGPR file), 16-byte aligned
// rows, every tensor < 4 GiB (32-bit buffer offsets), row-bias groups that are multiples of 64 rows.  Anything else goes to
// linear_kernel (linear.hip), which handles ragged edges.
#pragma once
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "linear.h"
#include "profile.h"

// Epilogue operands are read once and results are not re-read before >= 100 MB of other traffic has passed: non-temporal
// (no allocation in the L2 / MALL ahead of the activation panels); +1 % on the whole step (A/B on one device, round 2).
#define ARDAE_NT_LD " nt"
#define ARDAE_NT_ST " nt"
namespace ardae {
namespace wide {

constexpr int WBM = 64;                       // rows per tile
constexpr int WLDW = 68;                      // LDS row stride (floats): conflict-free ds_read_b128 fragments
constexpr int WBUF_BYTES = WBM * WLDW * 4;    // one K panel (<= 64 wide)
constexpr int NBUF = 3;                       // panel ring

typedef __attribute__((address_space(3))) float lds_f32;

// s_nop 4: a scalar base that the compiler produced with a VALU instruction (v_readlane of a spilled SGPR, v_readfirstlane)
// needs 5 wait states before a VMEM instruction may read it; the hazard recogniser does not look inside inline asm
// (seen as a memory fault once SGPR spills appeared).  It costs issue cycles of this wave only, not matrix-pipe time.
template <int OFF>
__device__ __forceinline__ void gload4(f32x4& dst, unsigned voff, const float* sbase) {
  asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(dst) : "v"(voff), "s"(sbase), "n"(OFF) : "memory");
}
// (NOP = false would be legal where the base is known to be SALU-written, but a spilled SGPR comes back through
// v_readlane at the compiler's discretion, so the wait states stay everywhere)
template <int OFF, bool NOP = true>
__device__ __forceinline__ void gload1(float& dst, unsigned voff, const float* sbase) {
  if (NOP) asm volatile("s_nop 4\n\tglobal_load_dword %0, %1, %2 offset:%3" : "=v"(dst) : "v"(voff), "s"(sbase), "n"(OFF) : "memory");
  else asm volatile("global_load_dword %0, %1, %2 offset:%3" : "=v"(dst) : "v"(voff), "s"(sbase), "n"(OFF) : "memory");
}
template <bool NOP = true>
__device__ __forceinline__ void gstore1(unsigned voff, float v, float* sbase) {
  if (NOP) asm volatile("s_nop 4\n\tglobal_store_dword %0, %1, %2" ::"v"(voff), "v"(v), "s"(sbase) : "memory");
  else asm volatile("global_store_dword %0, %1, %2" ::"v"(voff), "v"(v), "s"(sbase) : "memory");
}
// Epilogue tensors (saved activations in, results out) are addressed through raw buffer descriptors: row base = ONE 32-bit
// scalar offset (one s_add per access, no 64-bit pointer arithmetic), per-lane part in one VGPR per tensor.  num_records = the
// tensor's bytes: an access outside of it is dropped by the hardware instead of faulting.
// The s_nop 4 in every vector-memory asm statement is NOT optional: when the compiler runs out of SGPRs it parks them in VGPR
// lanes and brings them back with v_readlane right before use; a scalar operand (descriptor, offset, base) written by the
// vector ALU needs 5 wait states before a VMEM instruction reads it, and the hazard recogniser does not look inside inline
// asm.  Seen twice: a memory fault from the saddr loads of the first version, and again from a buffer descriptor restored by
// v_readlane in the rolled tile loop of the K = 32 instantiations (one panel per tile: the compiler keeps ~60 induction
// SGPRs there) when the s_nop had been dropped from the buffer forms.  tools/check_kernel_registers.py enforces it.
typedef int i32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ i32x4 make_rsrc(const void* p, unsigned bytes) {
  const unsigned long long a = (unsigned long long)p;
  i32x4 r;
  r[0] = (int)(unsigned)a;
  r[1] = (int)((unsigned)(a >> 32) & 0xffffu);   // stride 0: raw buffer
  r[2] = (int)bytes;
  r[3] = 0x00020000;                             // gfx9 / CDNA: DATA_FORMAT = 32-bit
  return r;
}
// "+v": the destination is TIED to the register of the value it replaces (the previous tile's result, stored a few chunks
// earlier), so that an epilogue operand / result slot is one physical register for the whole kernel - no copies at the loop
// back-edge, and a register budget the compiler cannot exceed by renaming (NLT = NST = 2 needs 128 such slots)
// Slots are register PAIRS (two consecutive rows of an accumulator column: what the packed FP32 instructions of the epilogue
// arithmetic want); H = which half this dword lands in.
template <int OFF, int H>
__device__ __forceinline__ void bload1(f32x2& dst, unsigned voff, const i32x4& rsrc, unsigned soff) {
  asm volatile("s_nop 4\n\tbuffer_load_dword %0, %1, %2, %3 offen offset:%4" ARDAE_NT_LD : "+v"(dst[H]) : "v"(voff), "s"(rsrc), "s"(soff), "n"(OFF) : "memory");
}
__device__ __forceinline__ void bstore1(unsigned voff, float v, const i32x4& rsrc, unsigned soff) {
  asm volatile("s_nop 4\n\tbuffer_store_dword %0, %1, %2, %3 offen" ARDAE_NT_ST ::"v"(v), "v"(voff), "s"(rsrc), "s"(soff) : "memory");
}
template <int OFF>
__device__ __forceinline__ void lds_read4(f32x4& dst, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory");
}
template <int OFF>
__device__ __forceinline__ void lds_write4(unsigned addr, const f32x4& v) {
  asm volatile("ds_write_b128 %0, %1 offset:%2" ::"v"(addr), "v"(v), "n"(OFF) : "memory");
}
// counter waits that "produce" the registers they guard, so no consumer can be scheduled above them
template <int VM, int NX>
__device__ __forceinline__ void wait_panel(f32x4 (&x)[NX]) {
  if (NX == 4) asm volatile("s_waitcnt vmcnt(%4)" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]) : "n"(VM) : "memory");
  else asm volatile("s_waitcnt vmcnt(%2)" : "+v"(x[0]), "+v"(x[1]) : "n"(VM) : "memory");
}
template <int VM>
__device__ __forceinline__ void wait16(f32x2* v) {
  asm volatile("s_waitcnt vmcnt(%8)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]) : "n"(VM) : "memory");
}

// panel geometry for NCH chunks of 8 k: 2*NCH float4 per row, 256 / (2*NCH) rows per pass, NX passes
template <int NCH>
struct PanelGeo {
  static constexpr int C4 = 2 * NCH;
  static constexpr int RPP = 256 / C4;
  static constexpr int NX = WBM / RPP;
};


template <int NCH, int NX>
__device__ __forceinline__ void store_panel(const f32x4 (&xv)[NX], unsigned waddr) {
  using PG = PanelGeo<NCH>;
  lds_write4<0>(waddr, xv[0]);
  lds_write4<PG::RPP * WLDW * 4>(waddr, xv[1]);
  if (NX == 4) {
    lds_write4<2 * PG::RPP * WLDW * 4>(waddr, xv[2]);
    lds_write4<3 * PG::RPP * WLDW * 4>(waddr, xv[3]);
  }
}
template <int OFF>
__device__ __forceinline__ void bload4(f32x4& dst, unsigned voff, const i32x4& rsrc, unsigned soff) {
  asm volatile("s_nop 4\n\tbuffer_load_dwordx4 %0, %1, %2, %3 offen offset:%4" : "=v"(dst) : "v"(voff), "s"(rsrc), "s"(soff), "n"(OFF) : "memory");
}
// a 1-KiB fragment of the packed weight image straight into four AGPRs
__device__ __forceinline__ void gload4_agpr(f32x4& dst, unsigned voff, const float* sbase) {
  asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %1, %2" : "=a"(dst) : "v"(voff), "s"(sbase) : "memory");
}
// first tile only: the slab loads are still landing (in order) while the K loop starts - chunk g waits for ITS fragment
template <int VM, int NJ>
__device__ __forceinline__ void wait_slab(f32x4 (&b)[NJ]) {
  if constexpr (NJ == 2) asm volatile("s_waitcnt vmcnt(%2)" : "+a"(b[0]), "+a"(b[1]) : "n"(VM) : "memory");
  else asm volatile("s_waitcnt vmcnt(%1)" : "+a"(b[0]) : "n"(VM) : "memory");   // (the same variable twice would be two operands: copies)
}
// acc += A x B (one k-pair); FIRST: the tile's first MFMA of this accumulator (SrcC = 0, no zero-initialisation needed);
// LAST: the tile's very last MFMA.  The hazard recogniser does not see inline-asm MFMAs, and the compiler is free to put its own
// instructions (register copies of the accumulators, seen in the K = 512 instantiation) right behind the asm statement, so the
// 16-pass MFMA's 18 wait states before a vector-ALU read of its result are part of the SAME asm statement (the other
// accumulators' last MFMAs are older by 64 cycles each).
template <bool FIRST, bool LAST>
__device__ __forceinline__ void mfma_vab(f32x16& acc, float a, float b) {
  if (FIRST) asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %2, 0" : "=v"(acc) : "v"(a), "a"(b));
  else if (LAST) asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %2, %0\n\ts_nop 15\n\ts_nop 3" : "+v"(acc) : "v"(a), "a"(b));
  else asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "a"(b));
}

// The order in which chunk g = p * NCH + c of a tile issues its memory operations behind its 16 MFMAs:
//   2 fragment reads A(g + 1) | c == 0: NX panel loads (next panel) | c == XW: NX panel LDS writes
//   | deferred stores of the PREVIOUS tile | NJ row-bias loads | epilogue-operand loads of THIS tile
// (NJ = 32-column blocks per wave: 2 for K <= 256, 1 for K = 512 - the wave's slab is 32 NJ columns x K = at most 256 registers)
// Stores come first (chunks [0, GS)), operand loads after them (chunks [GS, GE)), in half-block order, into the registers
// the stores have just read; the last GE .. G chunks carry none, so that the last operand has landed when the K loop ends.
// chunks of the weight slab the AGPR file holds at a time (all of them, or a rolling window of 64 / NJ: see Sched::ROLL)
constexpr int wide_slots(int NCH, int NP, int NJ) { return (NJ * NCH * NP * 4 <= 256) ? NCH * NP : 64 / NJ; }

template <int NCH, int NP, int NJ, int NLT, int NST, bool HP>
struct Sched {
  static constexpr int NX = PanelGeo<NCH>::NX;
  static constexpr int G = NP * NCH;
  // ROLL (K = 1024: the slab, 32 NJ columns x K, is twice the AGPR file): the AGPRs hold a WINDOW of SLOTS chunks; chunk g reads slot
  // g % SLOTS and, one chunk later, that slot is reloaded with chunk g + SLOTS's fragment (of this tile's second half, or the next
  // tile's first) - NJ loads per chunk behind the MFMAs, as linear_chain_kernel reloads its next layer's slab
  static constexpr int SLOTS = wide_slots(NCH, NP, NJ);
  static constexpr bool ROLL = SLOTS < G;
  static constexpr bool DEFER = NP >= 2;                       // with a single panel per tile the epilogue stores at once
  static constexpr int NSTO = (DEFER && HP) ? 32 * NJ * NST : 0;    // HP: there is a previous tile whose results wait in registers
  static constexpr int NLD = 32 * NJ * NLT;
  static constexpr int XW = NCH - 3, BAR = NCH - 2;
  static constexpr int GE = G >= 16 ? G - 5 : G - 1;
  static constexpr int GS = (NSTO + NLD) == 0 ? 0 : NLD == 0 ? GE : (GE * NSTO + (NSTO + NLD) / 2) / (NSTO + NLD);
  static constexpr int GRB = NLD == 0 ? GE - 1 : GS;           // chunk of the two row-bias loads
  static constexpr int DS = GS > 0 ? GS : 1, DL = GE > GS ? GE - GS : 1;   // chunks that carry stores / loads
  static constexpr int st_lo(int g) { return g >= GS ? NSTO : NSTO * g / DS; }
  static constexpr int st_hi(int g) { return g >= GS ? NSTO : NSTO * (g + 1) / DS; }
  static constexpr int ld_lo(int g) { return g < GS ? 0 : g >= GE ? NLD : NLD * (g - GS) / DL; }
  static constexpr int ld_hi(int g) { return g < GS ? 0 : g >= GE ? NLD : NLD * (g - GS + 1) / DL; }
  static constexpr int n_rb(int g) { return g == GRB ? NJ : 0; }
  static constexpr int n_sl(int g) { return ROLL ? NJ : 0; }   // slab-window reloads (chunk g reloads the slot of chunk g - 1)
  static constexpr int vmem(int g) { return (st_hi(g) - st_lo(g)) + n_rb(g) + (ld_hi(g) - ld_lo(g)) + n_sl(g); }   // without the panel loads
  // vector-memory operations younger than the panel loads of chunk (p, 0) when chunk (p, XW) moves them to LDS
  static constexpr int vm_panel(int p) {
    int n = 0;
    for (int k = 0; k < XW; ++k) n += vmem(p * NCH + k);
    return n > 63 ? 63 : n;
  }
  // first tile (the prologue issues: first panel, then the slab in chunk order): vector-memory operations younger than the
  // slab fragment of chunk g = (p, c) when that chunk starts.  vmcnt retires in order, so capping at 63 only waits longer.
  static constexpr int vm_slab(int p, int c) {
    const int g = p * NCH + c;
    int n = ((ROLL ? SLOTS : G) - 1 - g) * NJ + NX * (c > 0 ? p + 1 : p);
    if (n < 0) n = 0;
    for (int k = 0; k < g; ++k) n += vmem(k);
    return n > 63 ? 63 : n;
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// Epilogue.  The accumulator of a 32x32 block puts column l&31 and rows (r&3) + 8(r>>2) + 4(l>>5) in lane l, so operands
// and results move as dwords: one instruction = two full 128-byte lines.  Addressing is the saddr form (row base in
// SGPRs, per-lane column offset in one VGPR per tensor): no vector-ALU work per access.
// F1 / F2:  EPI_ACT: F1 = score seed Y2, F2 = per-row scale (sigma column);  EPI_DACT: F1 = additive Q;  EPI_CHAIN: unused
// ---------------------------------------------------------------------------------------------------------------------
template <int EPI, int ACT, bool F1, bool F2, int NJ_ = 2>
struct WideEpi {
  static constexpr int NJ = NJ_;                           // 32-column blocks per wave
  static constexpr int NLT = EPI == EPI_ACT ? (F2 ? 1 : 0) : EPI == EPI_DACT ? (F1 ? 2 : 1) : 2;   // tensors loaded per element
  static constexpr int NST = EPI == EPI_ACT ? (F1 ? 2 : 1) : EPI == EPI_DACT ? 1 : 2;              // tensors stored per element
  static constexpr bool SIGMA_OPERAND = EPI == EPI_ACT;   // its one loaded operand (F2) is the per-row sigma
  static constexpr bool CHAIN = EPI == EPI_CHAIN;

  const LinArgs& a;
  unsigned vY, vY2, vL0, vL1, vRS, vC;   // per-lane byte offsets
  i32x4 rY, rY2, rL0, rL1, rRS;          // buffer descriptors: Y, Y2, first / second loaded tensor, per-row sigma
  unsigned sY, sY2, sL0, sL1;            // their row strides in bytes
  float bcol0, wsig0, wfc0; unsigned pad_; float bcol1, wsig1, wfc1;   // column operands of the wave's two 32-column blocks.  Scalars, and the two blocks' values NOT adjacent: as arrays (or adjacent floats) the compiler paired wsig0/wsig1 through a stack slot to feed op_sel broadcasts of the packed instructions
  int colw_loaded;

  __device__ __forceinline__ WideEpi(const LinArgs& a_, int lane) : a(a_), colw_loaded(-1) {
    const int l31 = lane & 31, hh = lane >> 5;
    vY = (unsigned)((4 * hh * a.ldY + l31) * 4);
    vY2 = NST == 2 ? (unsigned)((4 * hh * (a.Y2 ? a.ldY2 : a.ldY) + l31) * 4) : 0u;   // absent Y2 (fused chains): Y again
    vL0 = (EPI != EPI_ACT) ? (unsigned)((4 * hh * a.ldS + l31) * 4) : 0u;
    vL1 = (EPI == EPI_CHAIN) ? (unsigned)((4 * hh * a.ldR + l31) * 4) : (EPI == EPI_DACT && F1) ? (unsigned)((4 * hh * a.ldQ + l31) * 4) : 0u;
    vRS = (unsigned)(16 * hh);
    vC = (unsigned)(l31 * 4);
    bcol0 = bcol1 = wsig0 = wsig1 = wfc0 = wfc1 = 0.f;
    const unsigned M = (unsigned)a.M;
    const float* y2 = a.Y2 ? a.Y2 : a.Y;
    const int ld2 = a.Y2 ? a.ldY2 : a.ldY;
    sY = (unsigned)a.ldY * 4u; sY2 = (unsigned)ld2 * 4u;
    rY = make_rsrc(a.Y, M * sY);
    rY2 = make_rsrc(y2, M * sY2);
    const float* t0 = EPI != EPI_ACT ? a.S : a.Y;
    const float* t1 = EPI == EPI_CHAIN ? a.R : (EPI == EPI_DACT && F1) ? a.Q : a.Y;
    sL0 = (unsigned)(EPI != EPI_ACT ? a.ldS : a.ldY) * 4u;
    sL1 = (unsigned)(EPI == EPI_CHAIN ? a.ldR : (EPI == EPI_DACT && F1) ? a.ldQ : a.ldY) * 4u;
    rL0 = make_rsrc(t0, M * sL0);
    rL1 = make_rsrc(t1, M * sL1);
    rRS = make_rsrc((EPI == EPI_ACT && a.rowscale) ? a.rowscale : a.src[0].x, M * 4u);
  }

  // column-only operands (bias, sigma weight, fc weight of the score seed): once per column panel
  __device__ __forceinline__ void column_operands(int colw, int lane) {
    if (EPI != EPI_ACT || colw == colw_loaded) return;
    colw_loaded = colw;
    const int l31 = lane & 31;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int col = colw + 32 * j + l31;
      const float b = a.bias ? a.bias[col] : 0.f;
      const float w = (F2 && a.rowscale_w) ? a.rowscale_w[col] : 0.f;
      const float f = (F1 && a.R) ? a.R[col] : 0.f;
      if (j == 0) { bcol0 = b; wsig0 = w; wfc0 = f; } else { bcol1 = b; wsig1 = w; wfc1 = f; }
    }
  }

  // group row-bias of the tile (two columns per lane); a dummy in-bounds load when there is none keeps the counts static
  template <int JJ>
  __device__ __forceinline__ void issue_rowbias_one(float& rbj, int row0, int colw) const {
    const float* p = (EPI == EPI_ACT && a.rowbias) ? a.rowbias + (size_t)(row0 / a.rows_per_group) * a.rowbias_ld + colw
                                                     : a.Y + (size_t)row0 * a.ldY + colw;
    gload1<128 * JJ>(rbj, vC, p);
  }

  // results replace the operands in place: l0 <- Y, l1 <- Y2; one register pair = accumulator elements 2k, 2k + 1 of the half-block
  template <int HB>
  __device__ __forceinline__ void math(const f32x16& acc16, f32x2* l0, f32x2* l1, float brow, f32x2& csum) const {
    constexpr int J = HB >> 2, H = HB & 1;
    const float ws = J == 0 ? wsig0 : wsig1, nw = -(J == 0 ? wfc0 : wfc1);
    const f32x2 brow2 = {brow, brow}, wsig2 = {ws, ws}, nwfc2 = {nw, nw};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      f32x2 v;
      v[0] = acc16[8 * H + 2 * k];
      v[1] = acc16[8 * H + 2 * k + 1];
      f32x2 em;
      if (EPI == EPI_ACT) {
        f32x2 x = v + brow2;
        if (F2 && a.rowscale) x = l0[k] * wsig2 + x;
        const f32x2 y = act_fwd2<ACT>(x);
        if (NST == 2) l1[k] = (F1 && a.Y2) ? nwfc2 * act_d1_2<ACT>(y, em) : y;
        l0[k] = y;
      } else if (EPI == EPI_DACT) {
        // result IN PLACE (see EPI_CHAIN below): the final multiply-add is asm with the slot as a read-write operand
        const f32x2 d1 = act_d1_2<ACT>(l0[k], em);
        if (F1) asm volatile("v_pk_fma_f32 %0, %1, %2, %3" : "+v"(l0[k]) : "v"(v), "v"(d1), "v"(l1[k]));
        else asm volatile("v_pk_mul_f32 %0, %1, %2" : "+v"(l0[k]) : "v"(v), "v"(d1));
      } else {
        // both results IN PLACE, by construction: the final multiplies are asm with the slot as a read-write operand
        const f32x2 d1 = act_d1_2<ACT>(l0[k], em);                                  // em = 1 - s without cancellation
        const f32x2 vem = v * em;
        asm volatile("v_pk_mul_f32 %0, %1, %2" : "+v"(l0[k]) : "v"(v), "v"(d1));   // Y  = V s
        asm volatile("v_pk_mul_f32 %0, %1, %0" : "+v"(l1[k]) : "v"(vem));          // Y2 = V R (1 - s)
      }
      csum += l0[k];
    }
  }

  template <int HB>
  __device__ __forceinline__ void stores(const f32x2* y, const f32x2* y2, int row0, int colw) const {
    constexpr int J = HB >> 2, I = (HB >> 1) & 1, H = HB & 1;
    const unsigned r0 = (unsigned)(row0 + 32 * I + 16 * H), c4 = (unsigned)(colw + 32 * J) * 4u;
    unsigned oy = r0 * sY + c4;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      bstore1(vY, y[e >> 1][e & 1], rY, oy);
      oy += (e == 3) ? 5u * sY : sY;
    }
    if (NST == 2) {
      unsigned o2 = r0 * sY2 + c4;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        bstore1(vY2, y2[e >> 1][e & 1], rY2, o2);
        o2 += (e == 3) ? 5u * sY2 : sY2;
      }
    }
  }

  __device__ __forceinline__ void store_all(const f32x2* y, const f32x2* y2, int row0, int colw) const {
    stores<0>(y + 0, y2 + 0, row0, colw); stores<1>(y + 4, y2 + 4, row0, colw); stores<2>(y + 8, y2 + 8, row0, colw);
    stores<3>(y + 12, y2 + 12, row0, colw);
    if constexpr (NJ == 2) {
      stores<4>(y + 16, y2 + 16, row0, colw); stores<5>(y + 20, y2 + 20, row0, colw);
      stores<6>(y + 24, y2 + 24, row0, colw); stores<7>(y + 28, y2 + 28, row0, colw);
    }
  }

  template <int VM, bool STORE_NOW>
  __device__ __forceinline__ void run(f32x16 (&acc)[2][NJ], f32x2* l0, f32x2* l1, float (&rb)[NJ], int lane, int row0, int colw, int tile_row) const {
    // one wait for everything the epilogue reads (issued >= NCH/2 chunks ago)
    asm volatile("s_waitcnt vmcnt(%2)" : "+v"(rb[0]), "+v"(rb[NJ - 1]) : "n"(VM) : "memory");
    if (NLT >= 1) { wait16<VM>(l0); wait16<VM>(l0 + 8); if (NJ == 2) { wait16<VM>(l0 + 16); wait16<VM>(l0 + 24); } }
    if (NLT == 2) { wait16<VM>(l1); wait16<VM>(l1 + 8); if (NJ == 2) { wait16<VM>(l1 + 16); wait16<VM>(l1 + 24); } }
    const bool has_rb = EPI == EPI_ACT && a.rowbias != nullptr;
    const float br0 = bcol0 + (has_rb ? rb[0] : 0.f), br1 = bcol1 + (has_rb ? rb[NJ - 1] : 0.f);
    f32x2 csum[2] = {f32x2{0.f, 0.f}, f32x2{0.f, 0.f}};
    // one half-block at a time (the scheduler would otherwise interleave all 64 elements and run out of registers)
    math<0>(acc[0][0], l0 + 0, l1 + 0, br0, csum[0]); __builtin_amdgcn_sched_barrier(0);
    math<1>(acc[0][0], l0 + 4, l1 + 4, br0, csum[0]); __builtin_amdgcn_sched_barrier(0);
    math<2>(acc[1][0], l0 + 8, l1 + 8, br0, csum[0]); __builtin_amdgcn_sched_barrier(0);
    math<3>(acc[1][0], l0 + 12, l1 + 12, br0, csum[0]); __builtin_amdgcn_sched_barrier(0);
    if constexpr (NJ == 2) {
      math<4>(acc[0][1], l0 + 16, l1 + 16, br1, csum[1]); __builtin_amdgcn_sched_barrier(0);
      math<5>(acc[0][1], l0 + 20, l1 + 20, br1, csum[1]); __builtin_amdgcn_sched_barrier(0);
      math<6>(acc[1][1], l0 + 24, l1 + 24, br1, csum[1]); __builtin_amdgcn_sched_barrier(0);
      math<7>(acc[1][1], l0 + 28, l1 + 28, br1, csum[1]); __builtin_amdgcn_sched_barrier(0);
    }
    if (STORE_NOW) store_all(l0, l1, row0, colw);
    if (a.colsum != nullptr) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const float c1 = csum[j][0] + csum[j][1];
        const float c2 = c1 + __shfl_xor(c1, 32);
        if (lane < 32) a.colsum[(size_t)tile_row * a.Nout + colw + 32 * j + lane] = c2;
      }
    }
  }
};

// everything a chunk needs besides the register arrays
template <int NCH, class EPI_T>
struct PanelCtx {
  const EPI_T& epi;
  const i32x4& rX;                       // activation tensor
  unsigned xvoff, xstep, xsoff_next;     // per-lane offset, bytes between the NX row groups of a panel, scalar offset of the NEXT panel
  unsigned raddr, raddr_next, waddr_next;
  int row0, colw, prev_row0;             // prev_row0 < 0: no previous tile (nothing to store yet)
  const float* wslab;                    // ROLL: this wave's slab in the packed image (chunk-major), lane part in bvoff
  unsigned bvoff;
  int kch;
};

// One chunk: wait for its A fragments (LDS), then 8 NJ MFMAs with the chunk's memory instructions spread evenly behind them
// (an MFMA keeps the pipe busy for 64 cycles while the wave is free to issue; with one wave per SIMD nobody else would fill
// a gap, and more than a handful of instructions behind one MFMA is a gap).
template <int C, int P, int NCH, int NP, bool HP, bool FT, class EPI_T>
struct ChunkOps {
  using SC = Sched<NCH, NP, EPI_T::NJ, EPI_T::NLT, EPI_T::NST, HP>;
  static constexpr int NX = PanelGeo<NCH>::NX;
  static constexpr int NLT = EPI_T::NLT, NST = EPI_T::NST, NJ = EPI_T::NJ, NMF = 8 * EPI_T::NJ;   // NMF: MFMAs per chunk
  static constexpr int GC = P * NCH + C;
  static constexpr int n_a = 2, n_x = C == 0 ? NX : 0, n_w = C == SC::XW ? NX : 0, n_st = SC::st_hi(GC) - SC::st_lo(GC), n_rb = SC::n_rb(GC),
                       n_op = SC::ld_hi(GC) - SC::ld_lo(GC), n_sl = SC::n_sl(GC);
  static constexpr int o_a = 0, o_x = o_a + n_a, o_w = o_x + n_x, o_st = o_w + n_w, o_rb = o_st + n_st, o_op = o_rb + n_rb, o_sl = o_op + n_op,
                       total = o_sl + n_sl;
  static constexpr int SLOTS = SC::SLOTS;
  static constexpr int PER = (total + NMF - 1) / NMF;   // instructions behind each MFMA

  // running scalar byte offsets of the store / operand streams (bumped by one row per instruction)
  struct Ptrs {
    unsigned py, py2, p0, p1;
  };

  template <int K>
  static __device__ __forceinline__ void op(f32x4 (&A)[2][2], f32x4 (&Bw)[SC::SLOTS][EPI_T::NJ], f32x4 (&xv)[NX], f32x2* l0, f32x2* l1, float (&rb)[EPI_T::NJ],
                                            const PanelCtx<NCH, EPI_T>& x, Ptrs& q) {
    using PG = PanelGeo<NCH>;
    const EPI_T& ep = x.epi;
    if constexpr (K >= o_sl) {   // ROLL: the slot chunk GC - 1 has just read gets the fragment SLOTS chunks ahead (wrapping into the next tile)
      constexpr int j = K - o_sl, GP = (GC + SC::G - 1) % SC::G, GN = (GP + SLOTS) % SC::G;
      asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %1, %2" : "+a"(Bw[GP % SLOTS][j]) : "v"(x.bvoff), "s"(x.wslab + ((size_t)j * x.kch + GN) * 256) : "memory");
    } else if constexpr (K < o_x) {   // fragment read of the next chunk (chunk 0 of the next panel after the last one)
      constexpr int i = K - o_a;
      if constexpr (C + 1 < NCH) lds_read4<(C + 1) * 32 + i * 32 * WLDW * 4>(A[(C + 1) & 1][i], x.raddr);
      else lds_read4<i * 32 * WLDW * 4>(A[0][i], x.raddr_next);
    } else if constexpr (K < o_w) {
      constexpr int u = K - o_x;
      bload4<0>(xv[u], x.xvoff, x.rX, x.xsoff_next + (unsigned)u * x.xstep);
    } else if constexpr (K < o_st) {
      constexpr int u = K - o_w;
      if constexpr (u == 0) wait_panel<SC::vm_panel(P), NX>(xv);
      lds_write4<u * PG::RPP * WLDW * 4>(x.waddr_next, xv[u]);
    } else if constexpr (K < o_rb) {
      constexpr int idx = SC::st_lo(GC) + (K - o_st);                     // index in the previous tile's store sequence
      constexpr int HB = idx / (8 * NST), tns = (idx / 8) % NST, e = idx % 8;
      constexpr int J = HB >> 2, I = (HB >> 1) & 1, H = HB & 1;
      constexpr bool fresh = e == 0 || K == o_st;
      constexpr int roff = 32 * I + 16 * H + (e & 3) + 8 * (e >> 2);
      if constexpr (tns == 0) {
        if constexpr (fresh) q.py = (unsigned)(x.prev_row0 + roff) * ep.sY + (unsigned)(x.colw + 32 * J) * 4u;
        bstore1(ep.vY, l0[4 * HB + (e >> 1)][e & 1], ep.rY, q.py);
        q.py += (e == 3) ? 5u * ep.sY : ep.sY;
      } else {
        if constexpr (fresh) q.py2 = (unsigned)(x.prev_row0 + roff) * ep.sY2 + (unsigned)(x.colw + 32 * J) * 4u;
        bstore1(ep.vY2, l1[4 * HB + (e >> 1)][e & 1], ep.rY2, q.py2);
        q.py2 += (e == 3) ? 5u * ep.sY2 : ep.sY2;
      }
    } else if constexpr (K < o_op) {
      constexpr int k = K - o_rb;
      if constexpr (k == 0) ep.template issue_rowbias_one<0>(rb[0], x.row0, x.colw);
      else ep.template issue_rowbias_one<1>(rb[NJ - 1], x.row0, x.colw);
    } else if constexpr (K < o_sl) {
      constexpr int idx = SC::ld_lo(GC) + (K - o_op);                     // index in the tile's operand-load sequence
      constexpr int HB = idx / (8 * NLT), tns = (idx / 8) % NLT, e = idx % 8;
      constexpr int J = HB >> 2, I = (HB >> 1) & 1, H = HB & 1;
      constexpr bool fresh = e == 0 || K == o_op;                         // first load of its stream in this chunk: full offset
      constexpr int roff = 32 * I + 16 * H + (e & 3) + 8 * (e >> 2);      // row of element e inside the tile (without the lane part)
      if constexpr (EPI_T::SIGMA_OPERAND) {   // EPI_ACT with a per-row scale: sigma of the row
        constexpr int off = ((e & 3) + 8 * (e >> 2)) * 4;
        bload1<off, (e & 1)>(l0[4 * HB + (e >> 1)], ep.vRS, ep.rRS, (unsigned)(x.row0 + 32 * I + 16 * H) * 4u);
      } else if constexpr (tns == 0) {
        if constexpr (fresh) q.p0 = (unsigned)(x.row0 + roff) * ep.sL0 + (unsigned)(x.colw + 32 * J) * 4u;
        bload1<0, (e & 1)>(l0[4 * HB + (e >> 1)], ep.vL0, ep.rL0, q.p0);
        q.p0 += (e == 3) ? 5u * ep.sL0 : ep.sL0;
      } else {
        if constexpr (fresh) q.p1 = (unsigned)(x.row0 + roff) * ep.sL1 + (unsigned)(x.colw + 32 * J) * 4u;
        bload1<0, (e & 1)>(l1[4 * HB + (e >> 1)], ep.vL1, ep.rL1, q.p1);
        q.p1 += (e == 3) ? 5u * ep.sL1 : ep.sL1;
      }
    }
  }

  // the instructions behind MFMA S
  template <int S, int R = 0>
  static __device__ __forceinline__ void slot(f32x4 (&A)[2][2], f32x4 (&Bw)[SC::SLOTS][EPI_T::NJ], f32x4 (&xv)[NX], f32x2* l0, f32x2* l1, float (&rb)[EPI_T::NJ],
                                              const PanelCtx<NCH, EPI_T>& x, Ptrs& q) {
    if constexpr (R < PER && S * PER + R < total) {
      op<S * PER + R>(A, Bw, xv, l0, l1, rb, x, q);
      slot<S, R + 1>(A, Bw, xv, l0, l1, rb, x, q);
    }
  }

  template <int S>
  static __device__ __forceinline__ void steps(f32x16 (&acc)[2][EPI_T::NJ], f32x4 (&A)[2][2], f32x4 (&Bw)[wide_slots(NCH, NP, EPI_T::NJ)][EPI_T::NJ], f32x4 (&xv)[NX], f32x2* l0, f32x2* l1,
                                               float (&rb)[EPI_T::NJ], const PanelCtx<NCH, EPI_T>& x, Ptrs& q) {
    if constexpr (S < NMF) {
      constexpr int kq = S / (2 * NJ), i = (S / NJ) & 1, j = S % NJ;
      mfma_vab<GC == 0 && kq == 0, GC == NP * NCH - 1 && S == NMF - 1>(acc[i][j], A[C & 1][i][kq], Bw[GC % SLOTS][j][kq]);
      slot<S>(A, Bw, xv, l0, l1, rb, x, q);
      steps<S + 1>(acc, A, Bw, xv, l0, l1, rb, x, q);
    }
  }

  static __device__ __forceinline__ void run(f32x16 (&acc)[2][EPI_T::NJ], f32x4 (&A)[2][2], f32x4 (&Bw)[wide_slots(NCH, NP, EPI_T::NJ)][EPI_T::NJ], f32x4 (&xv)[NX], f32x2* l0, f32x2* l1,
                                             float (&rb)[EPI_T::NJ], const PanelCtx<NCH, EPI_T>& x) {
    // this chunk's fragments (and, at XW + 1, this wave's panel writes) have landed in / left for LDS
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(A[C & 1][0]), "+v"(A[C & 1][1]) : : "memory");
    // the chunk's weight fragment: still landing behind the prologue on the first tile; under ROLL every other chunk reads a slot that
    // was reloaded SLOTS - 1 chunks ago - at least 63 younger vector-memory operations (one reload per chunk and the panel loads), so
    // vmcnt(63) proves it has landed (vmcnt retires in order)
    if constexpr (FT && GC < SLOTS) wait_slab<SC::vm_slab(P, C), NJ>(Bw[GC % SLOTS]);
    else if constexpr (SC::ROLL) wait_slab<63, NJ>(Bw[GC % SLOTS]);
    if (C == SC::BAR) __builtin_amdgcn_s_barrier();
    Ptrs q{0u, 0u, 0u, 0u};
    steps<0>(acc, A, Bw, xv, l0, l1, rb, x, q);
  }
};

template <int P, int NCH, int NP, bool HP, bool FT, class EPI_T>
__device__ __forceinline__ void panel(f32x16 (&acc)[2][EPI_T::NJ], f32x4 (&A)[2][2], f32x4 (&Bw)[wide_slots(NCH, NP, EPI_T::NJ)][EPI_T::NJ], f32x4 (&xv)[PanelGeo<NCH>::NX], f32x2* l0, f32x2* l1,
                                      float (&rb)[EPI_T::NJ], const PanelCtx<NCH, EPI_T>& x) {
  ChunkOps<0, P, NCH, NP, HP, FT, EPI_T>::run(acc, A, Bw, xv, l0, l1, rb, x);
  ChunkOps<1, P, NCH, NP, HP, FT, EPI_T>::run(acc, A, Bw, xv, l0, l1, rb, x);
  ChunkOps<2, P, NCH, NP, HP, FT, EPI_T>::run(acc, A, Bw, xv, l0, l1, rb, x);
  ChunkOps<3, P, NCH, NP, HP, FT, EPI_T>::run(acc, A, Bw, xv, l0, l1, rb, x);
  if constexpr (NCH == 8) {
    ChunkOps<4, P, NCH, NP, HP, FT, EPI_T>::run(acc, A, Bw, xv, l0, l1, rb, x);
    ChunkOps<5, P, NCH, NP, HP, FT, EPI_T>::run(acc, A, Bw, xv, l0, l1, rb, x);
    ChunkOps<6, P, NCH, NP, HP, FT, EPI_T>::run(acc, A, Bw, xv, l0, l1, rb, x);
    ChunkOps<7, P, NCH, NP, HP, FT, EPI_T>::run(acc, A, Bw, xv, l0, l1, rb, x);
  }
}

// panels P .. NP-1 of one tile, straight-line: values defined by the asm loads must never meet at a control-flow join
// (the compiler would reconcile them with register copies - of registers whose loads are still in flight)
template <int P, int NCH, int NP, bool HP, bool FT, class EPI_T, class PX>
__device__ __forceinline__ void tile_panels(f32x16 (&acc)[2][EPI_T::NJ], f32x4 (&A)[2][2], f32x4 (&Bw)[wide_slots(NCH, NP, EPI_T::NJ)][EPI_T::NJ], f32x4 (&xv)[PanelGeo<NCH>::NX], f32x2* l0,
                                            f32x2* l1, float (&rb)[EPI_T::NJ], const EPI_T& epi, const i32x4& rX, unsigned xvoff, unsigned xstep, int& buf,
                                            unsigned rlane, unsigned wlane, int row0, int colw, int prev_row0, int tile, int tnext, const PX& panel_x,
                                            const float* wslab, unsigned bvoff, int kch) {
  if constexpr (P < NP) {
    constexpr bool lastp = P + 1 == NP;
    const int bnext = buf + 1 == NBUF ? 0 : buf + 1;
    const PanelCtx<NCH, EPI_T> x{epi, rX, xvoff, xstep, panel_x(lastp ? tnext : tile, lastp ? 0 : P + 1), rlane + buf * WBUF_BYTES, rlane + bnext * WBUF_BYTES,
                                 wlane + bnext * WBUF_BYTES, row0, colw, prev_row0, wslab, bvoff, kch};
    panel<P, NCH, NP, HP, FT>(acc, A, Bw, xv, l0, l1, rb, x);
    buf = bnext;
    tile_panels<P + 1, NCH, NP, HP, FT>(acc, A, Bw, xv, l0, l1, rb, epi, rX, xvoff, xstep, buf, rlane, wlane, row0, colw, prev_row0, tile, tnext, panel_x, wslab,
                                        bvoff, kch);
  }
}

// NP = K panels per tile (compile time: the tile body is one basic block).  grid % ncp == 0, so a workgroup keeps its
// column panel: the weight slab and the column-only epilogue operands are loaded once.
template <int NCH, int NP, int NJ, int EPI, int ACT, bool F1, bool F2>
// tpg > 0 ("group tiles"): the per-image row-bias groups are no multiple of the 64-row tile (nz_cdae 625 of the shipped recipes).  Tiles are
// then laid out per group - tpg = ceil(rows_per_group / 64) of them, the last one shifted back so that it ENDS with its group - so that no
// tile meets two images; the rows two tiles of a group share are computed (identically) and written twice, +2.4 % work at 625 rows.
__device__ __forceinline__ void wide_body(const LinArgs& a, int nrt, int ncp, int tpg) {
  using PG = PanelGeo<NCH>;
  using EPI_T = WideEpi<EPI, ACT, F1, F2, NJ>;
  using SC = Sched<NCH, NP, NJ, EPI_T::NLT, EPI_T::NST, true>;
  constexpr int NX = PG::NX, G = NP * NCH;
  static_assert(NCH % 2 == 0 && NCH >= 4, "fragment double buffer / XW, BAR chunks");
  constexpr int SLOTS = wide_slots(NCH, NP, NJ);   // chunks of the slab resident at a time (G, or a rolling window: Sched::ROLL)
  static_assert(NJ * SLOTS * 4 <= 256 && G % SLOTS == 0, "the slab window must fit the AGPR file");
  __shared__ float lds[NBUF * WBM * WLDW];

#ifdef ARDAE_STAMPS
  const unsigned long long r_kernel = __builtin_amdgcn_s_memrealtime();
#endif
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hh = lane >> 5;

  const unsigned lds0 = (unsigned)(uintptr_t)(lds_f32*)lds;
  const unsigned rlane = lds0 + (unsigned)((l31 * WLDW + hh * 4) * 4);                         // fragment reads
  const unsigned wlane = lds0 + (unsigned)(((tid / PG::C4) * WLDW + (tid % PG::C4) * 4) * 4);   // panel stores

  // Workgroup -> (column panel, row tiles).  With several column panels the workgroups that share a row tile (= read the same
  // activation rows) are placed on ONE XCD (blocks b and b + 8 share an XCD: MI355X_MICROARCH.md), so that the rows are fetched
  // from beyond the XCD's L2 once; speed only - any placement is correct.
  const int b = (int)blockIdx.x, nwg = (int)gridDim.x;
  const bool xcd_map = ncp > 1 && nwg % (8 * ncp) == 0;
  const int cp = xcd_map ? (b >> 3) % ncp : b % ncp;
  const int rt0 = xcd_map ? ((b >> 3) / ncp) * 8 + (b & 7) : b / ncp;
  const int rts = nwg / ncp;                                // row tiles advance by this much per round
  const int colw = (cp * 4 * NJ + wave * NJ) * 32;
  EPI_T epi(a, lane);
  epi.column_operands(colw, lane);

  // activation tensor: buffer descriptor, per-lane offset of a panel load, scalar offset of panel p of tile t
  const unsigned ldx4 = (unsigned)a.src[0].ld * 4u;
  const i32x4 rX = make_rsrc(a.src[0].x, (unsigned)a.M * ldx4);
  const unsigned xvoff = (unsigned)(tid / PG::C4) * ldx4 + (unsigned)(tid % PG::C4) * 16u;
  const unsigned xstep = (unsigned)PG::RPP * ldx4;
  auto tile_row0 = [&](int rt) -> int {
    if (tpg == 0) return rt * WBM;
    const int g = rt / tpg, j = rt - g * tpg;
    const int r = j * WBM, last = a.rows_per_group - WBM;
    return __builtin_amdgcn_readfirstlane(g * a.rows_per_group + (r < last ? r : last));
  };
  auto panel_x = [&](int rt, int p) -> unsigned { return (unsigned)tile_row0(rt) * ldx4 + (unsigned)(p * 8 * NCH) * 4u; };

  f32x4 A[2][2], Bw[SLOTS][NJ], xv[NX];
  f32x2 l0[16 * NJ], l1[16 * NJ];
  float rb[NJ];
#pragma unroll
  for (int i = 0; i < 16 * NJ; ++i) l0[i] = l1[i] = f32x2{0.f, 0.f};   // the slots' registers exist from here on (tied asm operands read them)
  int tile = rt0;   // row tile
  // ---- prologue: the wave's weight slab into its AGPRs, first panel into LDS buffer 0, fragment set 0 in flight
  const unsigned bvoff = (unsigned)lane * 16u;
  const int kch = a.src[0].K >> 3;
  const float* wslab = a.src[0].wp + (size_t)(cp * 4 * NJ + wave * NJ) * kch * 256;
  {
    const float* wp = wslab;
    const unsigned x0 = panel_x(tile, 0);
#pragma unroll
    for (int u = 0; u < NX; ++u) bload4<0>(xv[u], xvoff, rX, x0 + (unsigned)u * xstep);
#pragma unroll
    for (int g = 0; g < SLOTS; ++g) {
      gload4_agpr(Bw[g][0], bvoff, wp + (size_t)g * 256);
      if constexpr (NJ == 2) gload4_agpr(Bw[g][1], bvoff, wp + ((size_t)kch + g) * 256);
    }
    // the panel is older than the slab: it has landed when at most the NJ SLOTS slab loads are outstanding; the slab keeps
    // landing behind the first tile's MFMAs (ChunkOps<.., FT = true> waits per chunk)
    wait_panel<(NJ * SLOTS > 63 ? 63 : NJ * SLOTS), NX>(xv);
    store_panel<NCH, NX>(xv, wlane);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    lds_read4<0>(A[0][0], rlane);
    lds_read4<32 * WLDW * 4>(A[0][1], rlane);
  }
  int buf = 0;
  int prev_row0 = -1;
#ifdef ARDAE_STAMPS
  unsigned long long t_k = 0, t_e = 0;
  const unsigned long long t_begin = __builtin_amdgcn_s_memtime();
  const unsigned long long r_begin = __builtin_amdgcn_s_memrealtime();
#endif
  // one tile: K loop (with the previous tile's stores riding along when HP) + epilogue arithmetic
  auto do_tile = [&](auto ft_tag) {
    constexpr bool FT = decltype(ft_tag)::value, HP = SC::DEFER && !FT;
#ifdef ARDAE_STAMPS
    const unsigned long long T0 = __builtin_amdgcn_s_memtime();
#endif
    const int tr = tile;
    const int row0 = tile_row0(tr);
    const int tnext = tile + rts < nrt ? tile + rts : tile;   // none: re-touch this tile (never used)
    f32x16 acc[2][NJ];
    tile_panels<0, NCH, NP, HP, FT>(acc, A, Bw, xv, l0, l1, rb, epi, rX, xvoff, xstep, buf, rlane, wlane, row0, colw, prev_row0, tile, tnext, panel_x, wslab, bvoff,
                                    kch);
#ifdef ARDAE_STAMPS
    const unsigned long long T1 = __builtin_amdgcn_s_memtime();
    t_k += T1 - T0;
#endif
    // Nothing may be in flight across the epilogue: it is compiler-scheduled code under register pressure, and a spill or
    // copy of a register whose load has not landed would read garbage.  (The wait states between the last MFMA and the first
    // vector-ALU read of an accumulator are part of that MFMA's asm statement, mfma_vab<.., LAST>.)
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)"
                 : "+v"(A[0][0]), "+v"(A[0][1]), "+v"(acc[0][0]), "+v"(acc[0][NJ - 1]), "+v"(acc[1][0]), "+v"(acc[1][NJ - 1])
                 :
                 : "memory");
    epi.template run<0, !SC::DEFER>(acc, l0, l1, rb, lane, row0, colw, tr);
    if (SC::DEFER) prev_row0 = row0;
#ifdef ARDAE_STAMPS
    t_e += __builtin_amdgcn_s_memtime() - T1;
#endif
  };
  // the first tile has no predecessor whose stores could ride in its K loop: its own copy of the tile body
  do_tile(std::true_type{});
  for (tile += rts; tile < nrt; tile += rts) do_tile(std::false_type{});
  if (SC::DEFER && prev_row0 >= 0) epi.store_all(l0, l1, prev_row0, colw);
  // the last panel prefetched a (dummy) next panel: drain before the registers die
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#ifdef ARDAE_STAMPS
  if (a.tile_loss != nullptr && lane == 0) {
    unsigned long long* o = reinterpret_cast<unsigned long long*>(a.tile_loss) + ((size_t)blockIdx.x * 4 + wave) * 8;
    const unsigned long long r_end = __builtin_amdgcn_s_memrealtime();
    o[0] = t_k; o[1] = t_e; o[2] = __builtin_amdgcn_s_memtime() - t_begin; o[3] = r_end - r_begin;   // 100 MHz ticks
    o[4] = r_begin; o[5] = r_end; o[6] = r_kernel;
  }
#endif
}

template <int NCH, int NP, int NJ, int EPI, int ACT, bool F1, bool F2>
__global__ __launch_bounds__(256, 1) void linear_wide_kernel(const LinArgs a, int nrt, int ncp, int tpg) {
  wide_body<NCH, NP, NJ, EPI, ACT, F1, F2>(a, nrt, ncp, tpg);
}

// A RUN of row-local layers of one kind (each reading its predecessor's output; same shape, epilogue, activation, flags) in ONE launch,
// LAYER-major: the workgroup walks all its row tiles for layer l - exactly wide_body, the wave's weight slab loaded once per layer - and
// then goes on to layer l + 1, whose rows it has written itself (a workgroup keeps its row tiles and its column panel: nothing is handed
// over between workgroups, so there is no grid-wide dependency; its own stores are complete (vmcnt) and ordered by a workgroup barrier
// before its own loads of them).  Against one launch per layer this removes the dispatch ramp / drain and the wait for the slowest
// workgroup at every layer boundary; the arithmetic is the per-layer kernel's, bit for bit.  (linear_chain_kernel is the TILE-major form
// for few tiles per workgroup: it keeps the tile in LDS but reloads the slab per tile and layer.)
constexpr int WIDE_MAXL = 6;
struct WideLayers {
  int nl;
  LinArgs L[WIDE_MAXL];
};
template <int NCH, int NP, int NJ, int EPI, int ACT, bool F1, bool F2>
__global__ __launch_bounds__(256, 1) void linear_wide_layers_kernel(const WideLayers c, int nrt, int ncp, int tpg) {
  for (int l = 0; l < c.nl; ++l) {
    wide_body<NCH, NP, NJ, EPI, ACT, F1, F2>(c.L[l], nrt, ncp, tpg);      // ends with every wave's s_waitcnt vmcnt(0)
    __syncthreads();
  }
}

int wide_grid(int ntiles, int ncp);

template <int NCH, int NP, int NJ, int EPI, int ACT, bool F1, bool F2>
int launch_wide(const LinArgs& a, hipStream_t st) {
  const int ncp = a.Nout / (128 * NJ);
  // row-bias groups that are no multiple of the tile height: tiles per group (see the kernel); linear_wide_eligible admitted the shape
  const int tpg = (EPI == EPI_ACT && a.rowbias && a.rows_per_group % WBM) ? (a.rows_per_group + WBM - 1) / WBM : 0;
  const int nrt = tpg ? (a.M / a.rows_per_group) * tpg : a.M / WBM;
  const int ntiles = nrt * ncp;
  const int grid = wide_grid(ntiles, ncp);
  if (g_prof_enabled)      // spelled as rocprofv3 demangles the instantiation: bench.py joins this log with profiles/pmc_summary.json by name
    prof_begin_named(st, lin_cost(a, epi_tensors(a, EPI)), "linear_wide_kernel<%d, %d, %d, %d, %d, %s, %s>", NCH, NP, NJ, EPI, ACT, F1 ? "true" : "false",
                     F2 ? "true" : "false");
  hipLaunchKernelGGL((linear_wide_kernel<NCH, NP, NJ, EPI, ACT, F1, F2>), dim3(grid), dim3(256), 0, st, a, nrt, ncp, tpg);
  prof_end(st);
  ARDAE_LAUNCH_CHECK();
  return 0;
}


template <int NCH, int NP, int NJ, int EPI, int ACT, bool F1, bool F2>
int launch_wide_layers(const LinArgs* L, int nl, hipStream_t st) {
  const LinArgs& a = L[0];
  const int ncp = a.Nout / (128 * NJ);
  const int nrt = a.M / WBM;
  const int grid = wide_grid(nrt * ncp, ncp);
  WideLayers c;
  memset(&c, 0, sizeof(c));
  c.nl = nl;
  for (int l = 0; l < nl; ++l) c.L[l] = L[l];
  if (g_prof_enabled)
    prof_begin_named(st, lin_cost_sum(L, nl, [](const LinArgs& l) { return epi_tensors(l, EPI); }), "linear_wide_layers_kernel<%d, %d, %d, %d, %d, %s, %s> x%d", NCH,
                     NP, NJ, EPI, ACT, F1 ? "true" : "false", F2 ? "true" : "false", nl);
  hipLaunchKernelGGL((linear_wide_layers_kernel<NCH, NP, NJ, EPI, ACT, F1, F2>), dim3(grid), dim3(256), 0, st, c, nrt, ncp, 0);
  prof_end(st);
  ARDAE_LAUNCH_CHECK();
  return 0;
}

// the layer runs of the cDAE update at h = 256: A_2.., the score pass (DACT), the forward-mode pass (CHAIN), the backward pass (DACT + Q)
#define ARDAE_WIDE_LAYERS_FOR(X)                          \
  X(8, 4, 2, EPI_ACT, ACT_SOFTPLUS, false, false)         \
  X(8, 4, 2, EPI_ACT, ACT_RELU, false, false)             \
  X(8, 4, 2, EPI_DACT, ACT_SOFTPLUS, false, false)        \
  X(8, 4, 2, EPI_DACT, ACT_SOFTPLUS, true, false)         \
  X(8, 4, 2, EPI_DACT, ACT_RELU, false, false)            \
  X(8, 4, 2, EPI_DACT, ACT_RELU, true, false)             \
  X(8, 4, 2, EPI_CHAIN, ACT_SOFTPLUS, false, false)
#define ARDAE_WIDE_LAYERS_EXTERN(NCH, NP, NJ, EPI, ACT, F1, F2) extern template int launch_wide_layers<NCH, NP, NJ, EPI, ACT, F1, F2>(const LinArgs*, int, hipStream_t);
#define ARDAE_WIDE_LAYERS_INSTANTIATE(NCH, NP, NJ, EPI, ACT, F1, F2) template int launch_wide_layers<NCH, NP, NJ, EPI, ACT, F1, F2>(const LinArgs*, int, hipStream_t);
#ifndef ARDAE_WIDE_INST_TU
ARDAE_WIDE_LAYERS_FOR(ARDAE_WIDE_LAYERS_EXTERN)
#endif

// explicit instantiations live in linear_wide_inst_*.hip
#define ARDAE_WIDE_FOR_GEOS(X, EPI, ACT, F1, F2) \
  X(8, 4, 2, EPI, ACT, F1, F2)                    \
  X(4, 1, 2, EPI, ACT, F1, F2)                    \
  X(8, 8, 1, EPI, ACT, F1, F2)
#define ARDAE_WIDE_FOR_ACT_FLAGS(X, ACT)          \
  ARDAE_WIDE_FOR_GEOS(X, EPI_ACT, ACT, false, false) \
  ARDAE_WIDE_FOR_GEOS(X, EPI_ACT, ACT, false, true)  \
  ARDAE_WIDE_FOR_GEOS(X, EPI_ACT, ACT, true, false)  \
  ARDAE_WIDE_FOR_GEOS(X, EPI_ACT, ACT, true, true)
#define ARDAE_WIDE_FOR_DACT_FLAGS(X, ACT)          \
  ARDAE_WIDE_FOR_GEOS(X, EPI_DACT, ACT, false, false) \
  ARDAE_WIDE_FOR_GEOS(X, EPI_DACT, ACT, true, false)
// K = 1024 (rolling slab window): the N-row layers of config #5 (mlp-res h 1024: forward layers incl. the one with the per-image
// row bias + sigma term, backward DACT without Q), softplus
#define ARDAE_WIDE_FOR_K1024(X)                        \
  X(8, 16, 1, EPI_ACT, ACT_SOFTPLUS, false, false)     \
  X(8, 16, 1, EPI_ACT, ACT_SOFTPLUS, false, true)      \
  X(8, 16, 1, EPI_DACT, ACT_SOFTPLUS, false, false)
#define ARDAE_WIDE_EXTERN(NCH, NP, NJ, EPI, ACT, F1, F2) extern template int launch_wide<NCH, NP, NJ, EPI, ACT, F1, F2>(const LinArgs&, hipStream_t);
#define ARDAE_WIDE_INSTANTIATE(NCH, NP, NJ, EPI, ACT, F1, F2) template int launch_wide<NCH, NP, NJ, EPI, ACT, F1, F2>(const LinArgs&, hipStream_t);
#ifndef ARDAE_WIDE_INST_TU
ARDAE_WIDE_FOR_ACT_FLAGS(ARDAE_WIDE_EXTERN, ACT_NONE)
ARDAE_WIDE_FOR_ACT_FLAGS(ARDAE_WIDE_EXTERN, ACT_RELU)
ARDAE_WIDE_FOR_ACT_FLAGS(ARDAE_WIDE_EXTERN, ACT_SOFTPLUS)
ARDAE_WIDE_FOR_DACT_FLAGS(ARDAE_WIDE_EXTERN, ACT_NONE)
ARDAE_WIDE_FOR_DACT_FLAGS(ARDAE_WIDE_EXTERN, ACT_RELU)
ARDAE_WIDE_FOR_DACT_FLAGS(ARDAE_WIDE_EXTERN, ACT_SOFTPLUS)
ARDAE_WIDE_FOR_GEOS(ARDAE_WIDE_EXTERN, EPI_CHAIN, ACT_SOFTPLUS, false, false)
ARDAE_WIDE_FOR_K1024(ARDAE_WIDE_EXTERN)
#endif

}  // namespace wide
}  // namespace ardae
