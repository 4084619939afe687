// The Legendre modal filter and the smoothness sensor of libtpsrhs.so (modal.hpp holds the operation and the plan):
// tpsrhs_modal_transform, tpsrhs_modal_energy, tpsrhs_modal_filter_apply, tpsrhs_modal_filter_configure,
// tpsrhs_modal_filter_read, and the two functions the device time loop calls after the stages of a step (abi_support.hpp:
// modal_filter_active, modal_filter_apply).
//
// Shape of the kernels.  One block is one wave of 64 lanes and owns EPB consecutive elements at a time (as many as fill the
// wave with nodes: lattice.hpp's rule; the last group of the mesh may hold fewer), the grid is capped and strides over the
// groups.  A row of the group's elements is ONE contiguous run of the field: it goes through registers into LDS, the N1 x N1
// matrix is applied one direction after the other (each pass: the lanes stride over the values of the tile, N1 multiply-adds
// from LDS each), and the last pass leaves the results in the registers of the lanes that loaded the same nodes -- so the
// difference u - u~ of the mean correction needs no second read, and every row is read once and written once.
//   contract<DIM, P>        the passes, shared by the three kernels; the matrix sits in LDS (one load per lane out of the
//                           kernel-argument segment)
//   k_modal_apply<DIM, P>   forward transform, inverse transform or a plain filter: whichever matrix it is given
//   k_modal_energy<DIM, P>  the forward transform, then the p + 1 shell sums: first along the lines of the first direction
//                           (a line lies in one shell up to i = max(j, k) and in shell i beyond), then over the lines
//   k_modal_filter<DIM, P>  the filter of the time loop, ONE launch per application: per group the sensor of sensor_row (the
//                           two steps of k_modal_energy on the incoming row), the decision, the weights and sum W, then row
//                           after row the contraction and the mean correction.  The next row is fetched while this one is
//                           contracted.  An element that is not filtered is neither read (beyond its sensor row) nor written.
// Sums over an element: with one element per block a butterfly over the wave's lanes; with several a round trip through LDS,
// every lane of an element adding the same numbers in the same order -- no floating-point atomic anywhere.  Counters: 64-bit
// integers summed per block in LDS, then one integer atomic per block and non-zero counter, as k_limit does.
#include "abi_support.hpp"
#include "quadrature_points.hpp"  // before modal.hpp: TPSRHS_HOST_DEVICE is defined there
#include "modal.hpp"

struct tpsrhs_modal_state {
  DevBuf<unsigned long long> d_counters;  // [MODAL_NCOUNTERS]
  ModalBasis basis;                       // V, V^-1 and gamma of the operator's order and nodes
  bool active = false;                    // tpsrhs_modal_filter_configure: the time loop applies `plan` after every step
  ModalPlan plan;
  ModalMatrix F = {};                     // of `plan`
};

namespace {

constexpr int MODAL_BLOCK = 64;        // one wave: the barriers between the passes cost next to nothing
constexpr int MODAL_MAXBLOCKS = 8192;  // eight waves on each of the four SIMDs of the 256 CUs

struct ModalGamma {
  double g[MODAL_MAXN1];
};

template <int DIM, int P>
struct Shape {
  static constexpr int N1 = P + 1;
  static constexpr int NPE = ipow(N1, DIM);
  static constexpr int LINES = NPE / N1;                                  // lines of the first direction per element
  static constexpr int EPB = NPE >= MODAL_BLOCK ? 1 : MODAL_BLOCK / NPE;  // 2-D: 16, 7, 4, 2, 1 for p = 1..5; 3-D: 8, 2, 1, 1, 1
  static constexpr int TILE = EPB * NPE;                                  // 64, 63, 64, 50, 36; 64, 54, 64, 125, 216
  static constexpr int TL = (TILE + MODAL_BLOCK - 1) / MODAL_BLOCK;       // tile values per lane
  static_assert(N1 * N1 <= MODAL_BLOCK, "one lane per entry of the matrix");
  static_assert(EPB * N1 <= MODAL_BLOCK, "one lane per element and shell");
};

// the leading N1 x N1 entries of a matrix out of the kernel argument into LDS: one load per lane from the kernel-argument
// segment (an unrolled select chain, as k_lattice has, pulls all 36 doubles of two matrices into scalar registers at once
// and spilled 16 of them at p = 5)
template <int N1>
__device__ __forceinline__ void stage_matrix(const ModalMatrix &M, double *sM, int tid) {
  if (tid < N1 * N1) sM[tid] = M.m[tid];
}
template <int N1>
__device__ __forceinline__ void stage_gamma(const ModalGamma &G, double *sg, int tid) {
  double v = 0.0;
#pragma unroll
  for (int t = 0; t < N1; t++) v = tid == t ? G.g[t] : v;
  if (tid < N1) sg[tid] = v;
}

// r[q] = ((M x ... x M) su)[tid + 64 q] for the ntile values the caller has just written to su (0 beyond them).  Starts with
// the barrier that makes su (and, the first time, sM) visible; when it returns su and v1 (3-D) may be written again, v1
// (2-D) / v2 (3-D) after the next barrier.
template <int DIM, int P>
__device__ __forceinline__ void contract(const double *sM, const double *su, double *v1, double *v2, int ntile, int tid,
                                         double (&r)[Shape<DIM, P>::TL]) {
  using S = Shape<DIM, P>;
  constexpr int N1 = S::N1, TL = S::TL;
  __syncthreads();
  // direction 0: v1[R][a] = sum_i M[a][i] su[R][i], R = (slot, k, j)
#pragma unroll
  for (int q = 0; q < TL; q++) {
    const int idx = tid + q * MODAL_BLOCK;
    if (idx < ntile) {
      const int R = idx / N1, a = idx - R * N1;
      const double *u = su + R * N1, *w = sM + a * N1;
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < N1; i++) s += w[i] * u[i];
      v1[idx] = s;
    }
  }
  __syncthreads();
  // direction 1: [S][b][a] = sum_j M[b][j] v1[S][j][a], S = (slot, k)
#pragma unroll
  for (int q = 0; q < TL; q++) {
    const int idx = tid + q * MODAL_BLOCK;
    double s = 0.0;
    if (idx < ntile) {
      const int a = idx % N1, b = (idx / N1) % N1, Sk = idx / (N1 * N1);
      const double *u = v1 + Sk * N1 * N1 + a, *w = sM + b * N1;
#pragma unroll
      for (int j = 0; j < N1; j++) s += w[j] * u[j * N1];
      if constexpr (DIM == 3) v2[idx] = s;
    }
    r[q] = s;
  }
  if constexpr (DIM == 3) {
    __syncthreads();
    // direction 2: [slot][c][b][a] = sum_k M[c][k] v2[slot][k][b][a]
#pragma unroll
    for (int q = 0; q < TL; q++) {
      const int idx = tid + q * MODAL_BLOCK;
      double s = 0.0;
      if (idx < ntile) {
        const int ab = idx % (N1 * N1), c = (idx / (N1 * N1)) % N1, slot = idx / S::NPE;
        const double *u = v2 + slot * S::NPE + ab, *w = sM + c * N1;
#pragma unroll
        for (int k = 0; k < N1; k++) s += w[k] * u[k * N1 * N1];
      }
      r[q] = s;
    }
  }
}

// sE[slot * N1 + m] = E_m of the group's elements from the modal coefficients c (contract's results); su and v1 are scratch.
// Ends with a barrier: sE may be read, su and v1 written.
template <int DIM, int P>
__device__ __forceinline__ void shell_energies(const double (&c)[Shape<DIM, P>::TL], const double *sg, double *su, double *v1,
                                               double *sE, int nel, int ntile, int tid) {
  using S = Shape<DIM, P>;
  constexpr int N1 = S::N1, TL = S::TL, LINES = S::LINES;
#pragma unroll
  for (int q = 0; q < TL; q++) {
    const int idx = tid + q * MODAL_BLOCK;
    if (idx < ntile) {
      const int i = idx % N1, j = (idx / N1) % N1, k = DIM == 3 ? (idx / (N1 * N1)) % N1 : 0;
      su[idx] = modal_mode_energy(c[q], modal_mode_weight(sg[i], sg[j], DIM == 3 ? sg[k] : 1.0));
    }
  }
  __syncthreads();  // (su was last read in contract's first pass, v1 before this barrier)
  // along a line (j, k fixed): the modes i <= max(j, k) lie in shell max(j, k), the mode i beyond it in shell i
  for (int ln = tid; ln < nel * LINES; ln += MODAL_BLOCK) {
    const int within = ln % LINES, j = within % N1, k = DIM == 3 ? within / N1 : 0, mjk = j > k ? j : k;
    double L[N1], acc = 0.0;
#pragma unroll
    for (int i = 0; i < N1; i++) {
      L[i] = su[ln * N1 + i];
      if (i <= mjk) acc += L[i];
    }
#pragma unroll
    for (int m = 0; m < N1; m++) v1[ln * N1 + m] = m < mjk ? 0.0 : (m == mjk ? acc : L[m]);
  }
  __syncthreads();
  if (tid < nel * N1) {
    const int slot = tid / N1, m = tid - slot * N1;
    double s = 0.0;
    for (int ln = 0; ln < LINES; ln++) s += v1[(slot * LINES + ln) * N1 + m];
    sE[tid] = s;
  }
  __syncthreads();
}

// S of element `slot` of the group from sE
template <int N1>
__device__ __forceinline__ double sensor_of(const double *sE, int slot) {
  double sum = 0.0;
#pragma unroll
  for (int m = 0; m < N1; m++) sum += sE[slot * N1 + m];
  return modal_sensor(sE[slot * N1 + N1 - 1], sum);
}

// the sum of d over the nodes of the lane's element (d: 0 beyond the tile); every lane of an element gets the same number
template <int DIM, int P>
__device__ __forceinline__ double element_sum(const double (&d)[Shape<DIM, P>::TL], double *sr, int ntile, int tid) {
  using S = Shape<DIM, P>;
  if constexpr (S::EPB == 1) {
    double v = 0.0;
#pragma unroll
    for (int q = 0; q < S::TL; q++) v += d[q];
#pragma unroll
    for (int off = MODAL_BLOCK / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, MODAL_BLOCK);
    return v;
  } else {
    static_assert(S::TL == 1, "several elements per block fit one value per lane");
    if (tid < ntile) sr[tid] = d[0];
    __syncthreads();
    double v = 0.0;
    if (tid < ntile) {
      const double *p = sr + (tid / S::NPE) * S::NPE;
      for (int n = 0; n < S::NPE; n++) v += p[n];
    }
    __syncthreads();  // sr may be written again
    return v;
  }
}

// in, out: [nrows][ndofs]; in == out allowed (a block reads a row of its elements completely before it writes it)
template <int DIM, int P>
__global__ void __launch_bounds__(MODAL_BLOCK)
    k_modal_apply(int ne, int nrows, int64_t ndofs, ModalMatrix M, const double *in, double *out) {
  using S = Shape<DIM, P>;
  constexpr int N1 = S::N1, NPE = S::NPE, EPB = S::EPB, TILE = S::TILE, TL = S::TL;
  __shared__ double sM[N1 * N1], su[TILE], v1[TILE], v2[DIM == 3 ? TILE : 1];
  const int tid = threadIdx.x;
  stage_matrix<N1>(M, sM, tid);
  const int64_t ngroups = (static_cast<int64_t>(ne) + EPB - 1) / EPB;
  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int64_t e0 = g * EPB, base = e0 * NPE;
    const int nel = static_cast<int>(ne - e0 < EPB ? ne - e0 : EPB);
    const int ntile = nel * NPE;
    double nxt[TL], r[TL];
#pragma unroll
    for (int q = 0; q < TL; q++) {
      const int idx = tid + q * MODAL_BLOCK;
      nxt[q] = idx < ntile ? in[base + idx] : 0.0;
    }
    for (int row = 0; row < nrows; row++) {
#pragma unroll
      for (int q = 0; q < TL; q++) {
        const int idx = tid + q * MODAL_BLOCK;
        if (idx < ntile) su[idx] = nxt[q];
      }
      if (row + 1 < nrows) {
        const double *src = in + (row + 1) * ndofs + base;
#pragma unroll
        for (int q = 0; q < TL; q++) {
          const int idx = tid + q * MODAL_BLOCK;
          if (idx < ntile) nxt[q] = src[idx];
        }
      }
      contract<DIM, P>(sM, su, v1, v2, ntile, tid, r);
      double *dst = out + row * ndofs + base;
#pragma unroll
      for (int q = 0; q < TL; q++) {
        const int idx = tid + q * MODAL_BLOCK;
        if (idx < ntile) dst[idx] = r[q];
      }
    }
    __syncthreads();  // the last pass has read v1 / v2 before the next group's passes write them
  }
}

// field: [ndofs]; energy_out: [ne][N1] or NULL; sensor_out: [ne] or NULL
template <int DIM, int P>
__global__ void __launch_bounds__(MODAL_BLOCK)
    k_modal_energy(int ne, ModalMatrix Vinv, ModalGamma G, const double *__restrict__ field, double *__restrict__ energy_out,
                   double *__restrict__ sensor_out) {
  using S = Shape<DIM, P>;
  constexpr int N1 = S::N1, NPE = S::NPE, EPB = S::EPB, TILE = S::TILE, TL = S::TL;
  __shared__ double sM[N1 * N1], sg[N1], su[TILE], v1[TILE], v2[DIM == 3 ? TILE : 1], sE[EPB * N1];
  const int tid = threadIdx.x;
  stage_matrix<N1>(Vinv, sM, tid);
  stage_gamma<N1>(G, sg, tid);
  const int64_t ngroups = (static_cast<int64_t>(ne) + EPB - 1) / EPB;
  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int64_t e0 = g * EPB, base = e0 * NPE;
    const int nel = static_cast<int>(ne - e0 < EPB ? ne - e0 : EPB);
    const int ntile = nel * NPE;
    double c[TL];
#pragma unroll
    for (int q = 0; q < TL; q++) {
      const int idx = tid + q * MODAL_BLOCK;
      if (idx < ntile) su[idx] = field[base + idx];
    }
    contract<DIM, P>(sM, su, v1, v2, ntile, tid, c);
    __syncthreads();  // 2-D: the last pass has read v1, which shell_energies writes
    shell_energies<DIM, P>(c, sg, su, v1, sE, nel, ntile, tid);
    if (energy_out && tid < nel * N1) energy_out[e0 * N1 + tid] = sE[tid];
    if (sensor_out && tid < nel) sensor_out[e0 + tid] = sensor_of<N1>(sE, tid);
    __syncthreads();  // sE has been read
  }
}

// x: [neq][ndofs], in place; w: [ndofs] (read only with pl.conservative)
template <int DIM, int P>
__global__ void __launch_bounds__(MODAL_BLOCK)
    k_modal_filter(int ne, int64_t ndofs, ModalPlan pl, ModalMatrix F, ModalMatrix Vinv, ModalGamma G, const double *__restrict__ w,
                   double *x, unsigned long long *__restrict__ counters) {
  using S = Shape<DIM, P>;
  constexpr int N1 = S::N1, NPE = S::NPE, EPB = S::EPB, TILE = S::TILE, TL = S::TL;
  __shared__ double sF[N1 * N1], sVi[N1 * N1], sg[N1], su[TILE], v1[TILE], v2[DIM == 3 ? TILE : 1], sE[EPB * N1];
  __shared__ double sr[EPB > 1 ? TILE : 1];
  __shared__ int sflag[EPB];
  __shared__ unsigned long long s_cnt[MODAL_NCOUNTERS];
  const int tid = threadIdx.x;
  stage_matrix<N1>(F, sF, tid);
  stage_matrix<N1>(Vinv, sVi, tid);
  stage_gamma<N1>(G, sg, tid);
  if (tid < MODAL_NCOUNTERS) s_cnt[tid] = 0;
  const int64_t ngroups = (static_cast<int64_t>(ne) + EPB - 1) / EPB;
  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const int64_t e0 = g * EPB, base = e0 * NPE;
    const int nel = static_cast<int>(ne - e0 < EPB ? ne - e0 : EPB);
    const int ntile = nel * NPE;
    // the decision, from the incoming sensor row, before anything is written
    if (pl.sensor_row >= 0) {
      const double *s = x + pl.sensor_row * ndofs + base;
      double c[TL];
#pragma unroll
      for (int q = 0; q < TL; q++) {
        const int idx = tid + q * MODAL_BLOCK;
        if (idx < ntile) su[idx] = s[idx];
      }
      contract<DIM, P>(sVi, su, v1, v2, ntile, tid, c);
      __syncthreads();  // 2-D: the last pass has read v1, which shell_energies writes
      shell_energies<DIM, P>(c, sg, su, v1, sE, nel, ntile, tid);
      if (tid < nel) sflag[tid] = modal_filtered(sensor_of<N1>(sE, tid), pl.sensor_threshold) ? 1 : 0;
    } else if (tid < nel) {
      sflag[tid] = 1;
    }
    __syncthreads();
    int nfiltered = 0;
    for (int s = 0; s < nel; s++) nfiltered += sflag[s];
    if (tid == 0) {  // the only writer of s_cnt inside the loop
      s_cnt[MODAL_SEEN] += static_cast<unsigned long long>(nel);
      s_cnt[MODAL_FILTERED] += static_cast<unsigned long long>(nfiltered);
    }
    bool mine[TL];
#pragma unroll
    for (int q = 0; q < TL; q++) {
      const int idx = tid + q * MODAL_BLOCK;
      mine[q] = idx < ntile && sflag[idx / NPE] != 0;
    }
    __syncthreads();  // sflag and sE have been read: the next group may write them
    if (nfiltered == 0) continue;  // the same for every lane
    double W[TL], sw = 0.0;
    if (pl.conservative) {
#pragma unroll
      for (int q = 0; q < TL; q++) W[q] = mine[q] ? w[base + tid + q * MODAL_BLOCK] : 0.0;
      sw = element_sum<DIM, P>(W, sr, ntile, tid);
    } else {
#pragma unroll
      for (int q = 0; q < TL; q++) W[q] = 0.0;
    }
    double nxt[TL], u[TL], r[TL];
    if (pl.num_rows > 0) {
      const double *v = x + pl.rows[0] * ndofs + base;
#pragma unroll
      for (int q = 0; q < TL; q++) nxt[q] = mine[q] ? v[tid + q * MODAL_BLOCK] : 0.0;
    }
    for (int i = 0; i < pl.num_rows; i++) {
#pragma unroll
      for (int q = 0; q < TL; q++) {
        const int idx = tid + q * MODAL_BLOCK;
        u[q] = nxt[q];
        if (idx < ntile) su[idx] = u[q];
      }
      if (i + 1 < pl.num_rows) {  // rows are distinct: the next row is not the one written below
        const double *v = x + pl.rows[i + 1] * ndofs + base;
#pragma unroll
        for (int q = 0; q < TL; q++) nxt[q] = mine[q] ? v[tid + q * MODAL_BLOCK] : 0.0;
      }
      contract<DIM, P>(sF, su, v1, v2, ntile, tid, r);
      if (pl.conservative) {
        double d[TL];
#pragma unroll
        for (int q = 0; q < TL; q++) d[q] = W[q] * (u[q] - r[q]);
        const double corr = modal_correction(element_sum<DIM, P>(d, sr, ntile, tid), sw);
#pragma unroll
        for (int q = 0; q < TL; q++) r[q] += corr;
      }
      double *v = x + pl.rows[i] * ndofs + base;
#pragma unroll
      for (int q = 0; q < TL; q++)
        if (mine[q]) v[tid + q * MODAL_BLOCK] = r[q];
    }
    __syncthreads();  // the last pass has read v1 / v2 before the next group's passes write them
  }
  __syncthreads();
  if (blockIdx.x == 0 && tid == 0) s_cnt[MODAL_CALLS] = 1;  // (this thread's own entry)
  if (tid == 0) {
    for (int i = 0; i < MODAL_NCOUNTERS; i++)
      if (s_cnt[i]) atomicAdd(&counters[i], s_cnt[i]);
  }
}

int modal_grid(const tpsrhs_operator *h, int epb) {
  const int64_t ngroups = (static_cast<int64_t>(h->ne) + epb - 1) / epb;
  return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(ngroups, MODAL_MAXBLOCKS)));
}

ModalGamma gamma_of(const ModalBasis &b) {
  ModalGamma g = {};
  for (int k = 0; k < b.n1; k++) g.g[k] = b.gamma[k];
  return g;
}

void nodes_of(const tpsrhs_operator *h, double *nodes) {
  double wts[TPSRHS_MAXORDER + 1];
  segment_rule01(h->nc, h->order + 1, nodes, wts);  // the nodes of the operator's basis, as lattice.hip takes them
}

// the state with the basis and the zeroed counters, at the first use; everything on the operator's stream
tpsrhs_modal_state *modal_of(tpsrhs_operator *h, const char *who) {
  if (h->modal) return h->modal.get();
  if (h->order < 1 || h->order > TPSRHS_MAXORDER || (h->dim != 2 && h->dim != 3))
    throw Unsupported(std::string(who) + ": dim 2 or 3 and polynomial orders 1..5 are built");
  std::unique_ptr<tpsrhs_modal_state> ms(new tpsrhs_modal_state());
  ms->d_counters = DevBuf<unsigned long long>(MODAL_NCOUNTERS);
  HIP_CHECK(hipMemsetAsync(ms->d_counters.get(), 0, sizeof(unsigned long long) * MODAL_NCOUNTERS, h->stream));
  double nodes[TPSRHS_MAXORDER + 1];
  nodes_of(h, nodes);
  ms->basis = modal_basis(h->nc, h->order + 1, nodes);
  h->modal = owned_state(std::move(ms));
  return h->modal.get();
}

ModalMatrix filter_matrix_of(const tpsrhs_operator *h, const ModalPlan &pl) {
  double nodes[TPSRHS_MAXORDER + 1];
  nodes_of(h, nodes);
  return modal_filter_matrix(h->nc, h->order + 1, nodes, pl.cutoff, pl.alpha, pl.exponent);
}

// one application on the operator's stream (an empty plan still counts as a call)
void apply(tpsrhs_operator *h, const tpsrhs_modal_state *ms, const ModalPlan &pl, const ModalMatrix &F, double *x) {
  const double *w = pl.conservative ? limiter_weights_device(h) : nullptr;
  const ModalGamma G = gamma_of(ms->basis);
  with_dim_order(h, "tpsrhs_modal_filter_apply", [&](auto dim, auto p) {
    constexpr int D = decltype(dim)::value, PP = decltype(p)::value;
    hipLaunchKernelGGL((k_modal_filter<D, PP>), dim3(modal_grid(h, Shape<D, PP>::EPB)), dim3(MODAL_BLOCK), 0, h->stream, h->ne,
                       h->ndofs, pl, F, ms->basis.Vinv, G, w, x, ms->d_counters.get());
  });
  HIP_CHECK(hipGetLastError());
}

}  // namespace

bool modal_filter_active(const tpsrhs_operator *h) { return h->modal && h->modal->active; }
void modal_filter_apply(tpsrhs_operator *h, double *x) { apply(h, h->modal.get(), h->modal->plan, h->modal->F, x); }

extern "C" {

int tpsrhs_modal_transform(tpsrhs_handle h, int inverse, int nrows, const double *in, double *out) {
  if (!h || !in || !out)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_modal_transform: needs a handle and the device arrays in and out");
  if (nrows < 1) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_modal_transform: nrows " + std::to_string(nrows) + " < 1");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    const tpsrhs_modal_state *ms = modal_of(h, "tpsrhs_modal_transform");
    const ModalMatrix &M = inverse ? ms->basis.V : ms->basis.Vinv;
    with_dim_order(h, "tpsrhs_modal_transform", [&](auto dim, auto p) {
      constexpr int D = decltype(dim)::value, PP = decltype(p)::value;
      hipLaunchKernelGGL((k_modal_apply<D, PP>), dim3(modal_grid(h, Shape<D, PP>::EPB)), dim3(MODAL_BLOCK), 0, h->stream, h->ne,
                         nrows, h->ndofs, M, in, out);
    });
    HIP_CHECK(hipGetLastError());
  });
}

int tpsrhs_modal_energy(tpsrhs_handle h, const double *field, double *energy_out, double *sensor_out) {
  if (!h || !field) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_modal_energy: needs a handle and the device array field");
  if (!energy_out && !sensor_out)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_modal_energy: energy_out and sensor_out are both NULL");
  return guarded([&] {
    HIP_CHECK(hipSetDevice(h->device));
    const tpsrhs_modal_state *ms = modal_of(h, "tpsrhs_modal_energy");
    const ModalGamma G = gamma_of(ms->basis);
    with_dim_order(h, "tpsrhs_modal_energy", [&](auto dim, auto p) {
      constexpr int D = decltype(dim)::value, PP = decltype(p)::value;
      hipLaunchKernelGGL((k_modal_energy<D, PP>), dim3(modal_grid(h, Shape<D, PP>::EPB)), dim3(MODAL_BLOCK), 0, h->stream, h->ne,
                         ms->basis.Vinv, G, field, energy_out, sensor_out);
    });
    HIP_CHECK(hipGetLastError());
  });
}

int tpsrhs_modal_filter_apply(tpsrhs_handle h, const tpsrhs_modal_filter *f, double *x) {
  if (!h || !f || !x)
    return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_modal_filter_apply: needs a handle, a filter and the device state x");
  return guarded([&] {
    const ModalPlan pl = plan_modal_filter(*f, h->neq, h->order, "tpsrhs_modal_filter_apply");
    HIP_CHECK(hipSetDevice(h->device));
    const tpsrhs_modal_state *ms = modal_of(h, "tpsrhs_modal_filter_apply");
    apply(h, ms, pl, filter_matrix_of(h, pl), x);
  });
}

int tpsrhs_modal_filter_configure(tpsrhs_handle h, const tpsrhs_modal_filter *f) {
  if (!h) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_modal_filter_configure: NULL handle");
  return guarded([&] {
    if (!f) {
      if (modal_filter_active(h)) {
        h->modal->active = false;
        h->loop.config_epoch++;
      }
      return;
    }
    const ModalPlan pl = plan_modal_filter(*f, h->neq, h->order, "tpsrhs_modal_filter_configure");
    HIP_CHECK(hipSetDevice(h->device));
    tpsrhs_modal_state *ms = modal_of(h, "tpsrhs_modal_filter_configure");
    if (pl.conservative) (void)limiter_weights_device(h);  // computed now: a step allocates nothing
    ms->plan = pl;
    ms->F = filter_matrix_of(h, pl);
    ms->active = true;
    h->loop.config_epoch++;  // a step graph captured before this call is not replayed (trace_chain.hpp)
  });
}

int tpsrhs_modal_filter_read(tpsrhs_handle h, tpsrhs_modal_filter_report *out, int reset) {
  if (!h || !out) return fail(TPSRHS_ERR_INVALID_ARGUMENT, "tpsrhs_modal_filter_read: needs a handle and the report");
  return guarded([&] {
    unsigned long long c[MODAL_NCOUNTERS] = {};
    HIP_CHECK(hipSetDevice(h->device));
    if (h->modal) {
      unsigned long long *d = h->modal->d_counters.get();
      HIP_CHECK(hipMemcpyAsync(c, d, sizeof(c), hipMemcpyDeviceToHost, h->stream));
      if (reset) HIP_CHECK(hipMemsetAsync(d, 0, sizeof(c), h->stream));
    }
    HIP_CHECK(hipStreamSynchronize(h->stream));
    *out = tpsrhs_modal_filter_report();
    out->calls = static_cast<int64_t>(c[MODAL_CALLS]);
    out->elements_seen = static_cast<int64_t>(c[MODAL_SEEN]);
    out->elements_filtered = static_cast<int64_t>(c[MODAL_FILTERED]);
  });
}

}  // extern "C"
