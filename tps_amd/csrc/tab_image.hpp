// The shape of a block (Cfg), the LDS copy of the 1-D tables that a block keeps (Tab) and its two makers: the lane-wise copy
// of kernels.hpp::load_tables as a function of the lane (tab_lane_copy: the same statements; load_tables keeps them written
// out, because a call, though inlined, moved the register allocation of kernels it should not touch) and the packed image the
// host builds once for the kernels with the staged prologue (make_tab_image).  Plain C++: the host test of the image compiles
// this header alone.
#ifndef TPSRHS_TAB_IMAGE_HPP_
#define TPSRHS_TAB_IMAGE_HPP_

#include "basis.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TPSRHS_HD __host__ __device__
#else
#define TPSRHS_HD
#endif

namespace tpsrhs {

// NC_ = 0: Gauss-Legendre basis + Gauss-Legendre rules (basisType 0, integrationRule 0): nodes and volume
//          quadrature points coincide, diagonal mass matrix -- the pair of the reference's cylinder / wedge / torch inputs;
// NC_ = 1: Gauss-Lobatto basis + Gauss-Lobatto rules (1, 1; the reference's defaults, src/M2ulPhyS.cpp:2671-2672):
//          p+2 volume points per direction, dense element mass matrix, every integral through quadrature points.
template <int DIM_, int P_, int NC_ = 0>
struct Cfg {
  static constexpr int DIM = DIM_, P = P_, N1 = P_ + 1, NC = NC_;
  static constexpr int NPE = (DIM_ == 3) ? N1 * N1 * N1 : N1 * N1;
  static constexpr int NF = (DIM_ == 3) ? N1 * N1 : N1;  // nodes of a face = lines through the element
  static constexpr int Q1 = ((DIM_ - 1) + 2 * P_) / 2 + 1 + NC_;  // face rule, order OrderW + 2p
  static constexpr int QV = P_ + 1 + NC_;                          // volume rule, order 2p
  static constexpr int NQV = (DIM_ == 3) ? QV * QV * QV : QV * QV;
  static constexpr int NQ = (DIM_ == 3) ? Q1 * Q1 : Q1;
  static constexpr int NW = (DIM_ == 3) ? Q1 * N1 : 1;  // half-interpolated face values (3-D only)
  static constexpr int NFACES = 2 * DIM_;
  static constexpr int NV = 1 << DIM_;
  // (the Gauss-Lobatto hexes of p = 2, 3 get two waves: their 100 / 72 face quadrature points per direction pair then
  // are ONE round of the block's lanes -- see EPB below)
  static constexpr int BLOCK = (NC_ && DIM_ == 3 && P_ >= 2) ? 128 : ((NPE <= 64) ? 64 : ((NPE <= 128) ? 128 : 256));
  // elements per block.  3-D p = 1: 3 elements = 54 face quadrature points per direction pair, one round of the
  // 64 lanes (4 elements needed a second round for 8 points, and with 11 equations that instantiation kept
  // 2 x 3 sets of prefetched traces live: 259 spilled VGPRs); the non-collocated pair has 16 points per face: 2
  // elements = 64 points, one round.  Round 2 ran that pair with 4 elements -- two rounds of face points in one wave,
  // the shape of round 2's failing 11-equation kernel -- and in round 3 the mixtures of 9+ equations with the argon
  // mixture transport returned a wrong species residual in the lanes of the block's third and fourth element, one of
  // them a memory fault (tools/probe_gll_p1.py): that shape is gone.
  // Every failing instantiation of rounds 2 and 3 had the same shape -- a single-wave block that takes TWO rounds of face
  // quadrature points (and then more than 256 registers with SGPR spills) --, and no other shape has failed in the
  // exhaustive sweep (tools/sweep_instantiations.py): in 3-D no block takes a second round any more.  Gauss-Lobatto
  // pair: p = 1: 2 hexes x 2 faces x 16 points = 64; p = 2: 2 hexes, 100 points, 128 lanes; p = 3: 1 hex, 72 points,
  // 128 lanes.  2-D, Gauss-Lobatto p = 1: 10 quads (60 points; 16 quads = 96 before).
  static constexpr int EPB = (DIM_ == 3 && NC_) ? (P_ == 3 ? 1 : 2)
                             : (DIM_ == 3 && P_ == 1) ? 3
                             : (DIM_ == 2 && NC_ && P_ == 1) ? 10
                                                             : BLOCK / NPE;
  static constexpr int NODES = EPB * NPE;
  // one direction pair (faces 2d, 2d+1) of a block
  static constexpr int PF = 2 * EPB;
  static constexpr int TN = PF * NF;
  static constexpr int TW = PF * NW;
  static constexpr int TQ = PF * NQ;
  static constexpr int LN = EPB * NF;
  static constexpr int Q_ROUNDS = (TQ + BLOCK - 1) / BLOCK;
  static_assert(DIM_ == 2 || Q_ROUNDS == 1, "3-D: one round of face quadrature points per direction pair");
  static_assert(!(DIM_ == 2 && NC_) || Q_ROUNDS == 1, "2-D Gauss-Lobatto pair: one round per direction pair");
  // 2-D: the quadrature points of BOTH direction pairs of a block are worked on together (at p = 3 they
  // are 2 x 32 = one full 64-lane round; one pair at a time leaves half of the lanes idle in the physics)
  static constexpr int TQ2 = 2 * TQ;
  static constexpr int Q2_ROUNDS = (TQ2 + BLOCK - 1) / BLOCK;
};

// LDS copy of the tables that are indexed per lane
template <class C>
struct Tab {
  double x[C::N1], w[C::N1], iw[C::N1], D[C::N1 * C::N1], b0[C::N1], b1[C::N1];
  double xq[C::Q1], wq[C::Q1], B[C::Q1 * C::N1];
  double xv[C::QV], wv[C::QV];  // volume rule (read by the non-collocated variant)
};

// what lane `tid` of the C::BLOCK lanes of a block copies from the tables of its (dim, order) into the block's Tab: statement
// for statement kernels.hpp::load_tables -- change the two together
template <class C>
TPSRHS_HD inline void tab_lane_copy(Tab<C> &t, const Tables1D &src, int tid) {
  if (tid < C::N1) {
    t.x[tid] = src.x[tid];
    t.w[tid] = src.w[tid];
    t.iw[tid] = 1.0 / src.w[tid];
    t.b0[tid] = src.b0[tid];
    t.b1[tid] = src.b1[tid];
  }
  if (tid < C::Q1) {
    t.xq[tid] = src.xq[tid];
    t.wq[tid] = src.wq[tid];
  }
  if (tid < C::QV) {
    t.xv[tid] = src.xv[tid];
    t.wv[tid] = src.wv[tid];
  }
  for (int i = tid; i < C::N1 * C::N1; i += C::BLOCK) t.D[i] = src.D[i];
  for (int i = tid; i < C::Q1 * C::N1; i += C::BLOCK) t.B[i] = src.B[i];
}

// The same Tab, every member, built on the host: the image a staged prologue copies to LDS word by word.  1 / w is an IEEE
// division here as on the device (the compiler's division sequence there is correctly rounded): the same bits.
template <class C>
inline Tab<C> make_tab_image(const Tables1D &src) {
  static_assert(sizeof(Tab<C>) == sizeof(double) * (5 * C::N1 + C::N1 * C::N1 + 2 * C::Q1 + C::Q1 * C::N1 + 2 * C::QV),
                "Tab<C> is doubles without padding: the image is copied as an array of them");
  Tab<C> t;
  for (int i = 0; i < C::N1; i++) {
    t.x[i] = src.x[i];
    t.w[i] = src.w[i];
    t.iw[i] = 1.0 / src.w[i];
    t.b0[i] = src.b0[i];
    t.b1[i] = src.b1[i];
  }
  for (int i = 0; i < C::Q1; i++) {
    t.xq[i] = src.xq[i];
    t.wq[i] = src.wq[i];
  }
  for (int i = 0; i < C::QV; i++) {
    t.xv[i] = src.xv[i];
    t.wv[i] = src.wv[i];
  }
  for (int i = 0; i < C::N1 * C::N1; i++) t.D[i] = src.D[i];
  for (int i = 0; i < C::Q1 * C::N1; i++) t.B[i] = src.B[i];
  return t;
}

}  // namespace tpsrhs
#endif
