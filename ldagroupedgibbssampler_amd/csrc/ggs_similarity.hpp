// ggs_similarity.hpp -- the distance classes of cc/mallet/similarity between the rows of two matrices, and the n nearest rows:
// what LDADistancer.distance (LDADistancer.java:79-99), the loop of tui/LDASimilarity.java:175-183 and
// KLDivergenceClassifier.classify (:71-78) compute on one thread, Q x D x K scalar steps.
//
// A [n][len] holds the v1 rows (training documents, class centroids), B [m][len] the v2 rows (queries): Distance.calculate(v1, v2)
// is always called that way round.  Each class is restated operation by operation: every sum starts at 0.0 and
// takes its addends in index order, every product, quotient and sum is rounded on its own (the unit is built with
// -ffp-contract=off), Math.pow(x, 2) is x * x, Math.log is strict_log, sqrt and / are correctly rounded.
//
// The tile body is ggs_distances.hpp's: 256 lanes (16 x 16) own T = 16 R rows of A against T rows of B, a lane R x R pairs, the
// index runs in chunks of KC staged k-major through LDS.  Here it is a template over a metric functor:
//   Acc                  a pair's accumulators
//   stage(v, aux)        what is staged for a row's element: the element, or a pure function of it and its row (Hellinger's
//                        sqrt(v[i]), the deviation v[i] - mean of StatisticalDistance): the same doubles as in Java, once per tile
//   step(acc, a, b, k)   index k of the pair's loops
//   finish(acc, auxA, auxB, len)   the value calculate() returns
// aux [rows][2] are a row's own quantities (sim_aux_kernel): sqrt(sum v^2) for Cosine, mean and variance for metrics 10 and 11.
// Rows past the end are staged as 0.0 and never read out.
//
// A workgroup owns a tile of queries and one of S segments of A's tiles and walks the segment.  After a tile's loops the R x R
// values of every lane go through LDS (the staging buffers, free by then) as [query][document]:
//   dense    out[q][d] is written from there, a query's row contiguous
//   nearest  one lane per query inserts the tile's documents in index order into the query's list of n (distance, index)
//            pairs, which lives in LDS for the whole segment; the lists [Q][S][n] are merged by sim_merge_kernel.
// The order is (distance rising by value, index rising): -0.0 == 0.0, a candidate must be < +inf (NaN and +inf never enter),
// unfilled places hold (+inf, -1).  It is total, so the result does not depend on S or on the order of the tiles.
// The length rule of LDADistancer.java:84-87 is part of the value: both documents empty 0.0, one of them +inf.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ggs_device_math.hpp"
#include "ggs_distances.hpp"

namespace ggs {

constexpr int kSimMetrics = 12;
constexpr int kSimKC = 32;                             // the chunk of the index
constexpr int kSimMaxNearest = 16;
constexpr int kSimMergeBlock = 64;
// pairs per lane edge by metric id (the tile edge is 16 R): one accumulator per pair at R = 4, up to nine at R = 2
constexpr int kSimR[kSimMetrics] = {4, 4, 4, 4, 4, 4, 4, 2, 2, 2, 4, 4};
enum { kSimAuxNone = 0, kSimAuxNorm = 1, kSimAuxMoments = 2 };

__device__ __forceinline__ double sim_inf() { return __longlong_as_double((long long)kDistInfBits); }
// java.lang.Math.max / min: either operand NaN gives NaN, -0.0 is below 0.0
__device__ __forceinline__ double java_max(double a, double b) {
  if (a != a) return a;
  if (a == 0.0 && b == 0.0 && __double_as_longlong(a) < 0) return b;
  return a >= b ? a : b;
}
__device__ __forceinline__ double java_min(double a, double b) {
  if (a != a) return a;
  if (a == 0.0 && b == 0.0 && __double_as_longlong(b) < 0) return b;
  return a <= b ? a : b;
}
constexpr double kSimLn2 = 0x1.62e42fefa39efp-1;       // Math.log(2) = 0x3FE62E42FEFA39EF

// One index of cc.mallet.util.Maths.klDivergence(p1, p2) as DESIGN.md 2 assumes it: p1 == 0 skips, p2 == 0 returns +inf at once
// (`inf` latches: whatever the sum holds by then or would take later is dropped), else klDiv += p1 * Math.log(p1 / p2).
struct KlSum {
  double s;
  uint32_t inf;
};
__device__ __forceinline__ void kl_init(KlSum &q) { q.s = 0.0; q.inf = 0; }
__device__ __forceinline__ void kl_step(KlSum &q, double p1, double p2) {
  if (p1 == 0.0) return;
  if (p2 == 0.0) { q.inf = 1; return; }
  q.s = q.s + p1 * strict_log_body(p1 / p2);
}
__device__ __forceinline__ double kl_finish(const KlSum &q) { return q.inf ? sim_inf() : q.s / kSimLn2; }

struct SimPlain {                                      // what most metrics stage and keep beside a row
  static constexpr int kAux = kSimAuxNone;
  static constexpr bool kLoop = true;
  static constexpr int kUnroll = 8;                    // of a full chunk's steps; 1 where a step holds a log
  static __device__ __forceinline__ double stage(double v, const double *) { return v; }
};
struct SimOneSum { double s; };

struct SimManhattan : SimPlain {
  static constexpr int R = kSimR[0];
  using Acc = SimOneSum;
  static __device__ __forceinline__ void init(Acc &q) { q.s = 0.0; }
  static __device__ __forceinline__ void step(Acc &q, double a, double b, int) { q.s = q.s + fabs(a - b); }
  static __device__ __forceinline__ double finish(const Acc &q, const double *, const double *, int64_t) { return q.s; }
};
struct SimEuclidian : SimPlain {
  static constexpr int R = kSimR[1];
  using Acc = SimOneSum;
  static __device__ __forceinline__ void init(Acc &q) { q.s = 0.0; }
  static __device__ __forceinline__ void step(Acc &q, double a, double b, int) { const double dp = a - b; q.s = q.s + dp * dp; }
  static __device__ __forceinline__ double finish(const Acc &q, const double *, const double *, int64_t) { return sqrt(q.s); }
};
struct SimHellinger : SimPlain {                       // the sum itself: no root, no 1/2, as written
  static constexpr int R = kSimR[2];
  using Acc = SimOneSum;
  static __device__ __forceinline__ double stage(double v, const double *) { return sqrt(v); }
  static __device__ __forceinline__ void init(Acc &q) { q.s = 0.0; }
  static __device__ __forceinline__ void step(Acc &q, double a, double b, int) { const double dp = a - b; q.s = q.s + dp * dp; }
  static __device__ __forceinline__ double finish(const Acc &q, const double *, const double *, int64_t) { return q.s; }
};
struct SimCosine : SimPlain {                          // aux[0] = Math.sqrt(norm) of the row
  static constexpr int R = kSimR[3];
  static constexpr int kAux = kSimAuxNorm;
  using Acc = SimOneSum;
  static __device__ __forceinline__ void init(Acc &q) { q.s = 0.0; }
  static __device__ __forceinline__ void step(Acc &q, double a, double b, int) { q.s = q.s + a * b; }
  static __device__ __forceinline__ double finish(const Acc &q, const double *xa, const double *xb, int64_t) { return 1 + (-(q.s / (xa[0] * xb[0]))); }
};
__device__ __forceinline__ double canberra_term(double a, double b) {
  const double num = fabs(a - b), denom = fabs(a) + fabs(b);
  return denom == 0.0 ? 0.0 : num / denom;
}
struct SimCanberra : SimPlain {
  static constexpr int R = kSimR[4];
  using Acc = SimOneSum;
  static __device__ __forceinline__ void init(Acc &q) { q.s = 0.0; }
  static __device__ __forceinline__ void step(Acc &q, double a, double b, int) { q.s = q.s + canberra_term(a, b); }
  static __device__ __forceinline__ double finish(const Acc &q, const double *, const double *, int64_t) { return q.s; }
};
struct SimChebychev : SimPlain {
  static constexpr int R = kSimR[5];
  using Acc = SimOneSum;
  static __device__ __forceinline__ void init(Acc &q) { q.s = 0.0; }
  static __device__ __forceinline__ void step(Acc &q, double a, double b, int) { q.s = java_max(q.s, fabs(a - b)); }
  static __device__ __forceinline__ double finish(const Acc &q, const double *, const double *, int64_t) { return q.s; }
};
struct SimTwoSums { double i, u; };
__device__ __forceinline__ double jaccard_value(double inter, double uni) { return inter > 0.0 ? 1 - (inter / uni) : 0.0; }
struct SimJaccard : SimPlain {
  static constexpr int R = kSimR[6];
  static constexpr int kUnroll = 2;                    // 32 sums and the selects of min and max: eight steps' worth passes 256 VGPRs
  using Acc = SimTwoSums;
  static __device__ __forceinline__ void init(Acc &q) { q.i = 0.0; q.u = 0.0; }
  static __device__ __forceinline__ void step(Acc &q, double a, double b, int) { q.i = q.i + java_min(a, b); q.u = q.u + java_max(a, b); }
  static __device__ __forceinline__ double finish(const Acc &q, const double *, const double *, int64_t) { return jaccard_value(q.i, q.u); }
};
struct SimKlPair { KlSum ab, ba; };
__device__ __forceinline__ double kl_distance(const KlSum &u1, const KlSum &u2) { return (kl_finish(u1) + kl_finish(u2)) / 2; }
struct SimKL : SimPlain {
  static constexpr int kUnroll = 1;
  static constexpr int R = kSimR[7];
  using Acc = SimKlPair;
  static __device__ __forceinline__ void init(Acc &q) { kl_init(q.ab); kl_init(q.ba); }
  static __device__ __forceinline__ void step(Acc &q, double a, double b, int) { kl_step(q.ab, a, b); kl_step(q.ba, b, a); }
  static __device__ __forceinline__ double finish(const Acc &q, const double *, const double *, int64_t) { return kl_distance(q.ab, q.ba); }
};
struct SimJsAcc { KlSum a_avg, avg_a, b_avg, avg_b; };
struct SimJensenShannon : SimPlain {                   // avg[i] += (v1[i] + v2[i]) / 2.0 on a fresh array
  static constexpr int kUnroll = 1;
  static constexpr int R = kSimR[8];
  using Acc = SimJsAcc;
  static __device__ __forceinline__ void init(Acc &q) { kl_init(q.a_avg); kl_init(q.avg_a); kl_init(q.b_avg); kl_init(q.avg_b); }
  static __device__ __forceinline__ void step(Acc &q, double a, double b, int) {
    const double avg = 0.0 + (a + b) / 2.0;
    kl_step(q.a_avg, a, avg); kl_step(q.avg_a, avg, a); kl_step(q.b_avg, b, avg); kl_step(q.avg_b, avg, b);
  }
  static __device__ __forceinline__ double finish(const Acc &q, const double *, const double *, int64_t) {
    return (kl_distance(q.a_avg, q.avg_a) + kl_distance(q.b_avg, q.avg_b)) / 2;
  }
};
struct SimUberAcc { double canberra, chebychev, dot, euclid, inter, uni, manhattan; KlSum ab, ba; };
struct SimUber : SimPlain {                            // Canberra, Chebychev, Cosine, Euclidian, Jaccard, KL, Manhattan, / 7
  static constexpr int kUnroll = 1;
  static constexpr int R = kSimR[9];
  static constexpr int kAux = kSimAuxNorm;
  using Acc = SimUberAcc;
  static __device__ __forceinline__ void init(Acc &q) {
    q.canberra = q.chebychev = q.dot = q.euclid = q.inter = q.uni = q.manhattan = 0.0;
    kl_init(q.ab); kl_init(q.ba);
  }
  static __device__ __forceinline__ void step(Acc &q, double a, double b, int) {
    const double dp = a - b, ad = fabs(dp);
    q.canberra = q.canberra + canberra_term(a, b);
    q.chebychev = java_max(q.chebychev, ad);
    q.dot = q.dot + a * b;
    q.euclid = q.euclid + dp * dp;
    q.inter = q.inter + java_min(a, b); q.uni = q.uni + java_max(a, b);
    kl_step(q.ab, a, b); kl_step(q.ba, b, a);
    q.manhattan = q.manhattan + ad;
  }
  static __device__ __forceinline__ double finish(const Acc &q, const double *xa, const double *xb, int64_t) {
    double sum = 0.0;
    sum = sum + q.canberra;
    sum = sum + q.chebychev;
    sum = sum + (1 + (-(q.dot / (xa[0] * xb[0]))));
    sum = sum + sqrt(q.euclid);
    sum = sum + jaccard_value(q.inter, q.uni);
    sum = sum + kl_distance(q.ab, q.ba);
    sum = sum + q.manhattan;
    return sum / 7;
  }
};
struct SimStatistical : SimPlain {                     // aux = {mean, variance}; staged: the deviation v[i] - mean
  static constexpr int R = kSimR[10];
  static constexpr int kAux = kSimAuxMoments;
  using Acc = SimOneSum;
  static __device__ __forceinline__ double stage(double v, const double *aux) { return v - aux[0]; }
  static __device__ __forceinline__ void init(Acc &q) { q.s = 0.0; }
  static __device__ __forceinline__ void step(Acc &q, double a, double b, int k) { q.s = q.s + (a * b - q.s) / (double)(k + 1); }
  static __device__ __forceinline__ double finish(const Acc &q, const double *xa, const double *xb, int64_t) {
    const double correlation = q.s / sqrt(xa[1] * xb[1]);
    return -(correlation - 1);
  }
};
struct SimBhattacharyya : SimPlain {                   // the rows' moments only: no loop over the index
  static constexpr int R = kSimR[11];
  static constexpr int kAux = kSimAuxMoments;
  static constexpr bool kLoop = false;
  using Acc = SimOneSum;
  static __device__ __forceinline__ void init(Acc &q) { q.s = 0.0; }
  static __device__ __forceinline__ void step(Acc &, double, double, int) {}
  static __device__ __forceinline__ double finish(const Acc &, const double *xa, const double *xb, int64_t) {
    const double of = 1.0 / 4.0, var1 = xa[1], var2 = xb[1], mean1 = xa[0], mean2 = xb[0];
    const double t1 = strict_log_body(of * (var1 / var2 + var2 / var2 + 2));
    const double dm = mean1 - mean2;
    const double t2 = (dm * dm) / (var1 + var2);
    return of * t1 + of * t2;
  }
};

// aux [rows][2] of rows [rows][len]: StatisticalDistance.mean / variance, or Math.sqrt of the Cosine norm; one lane per row
__global__ __launch_bounds__(256) void sim_aux_kernel(const double *__restrict__ rows, int64_t n, int64_t len, int kind, double *__restrict__ aux) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    const double *v = rows + r * len;
    if (kind == kSimAuxNorm) {
      double norm = 0.0;
      for (int64_t i = 0; i < len; ++i) norm = norm + v[i] * v[i];
      aux[2 * r] = sqrt(norm); aux[2 * r + 1] = 0.0;
    } else {
      double sum = 0.0;
      for (int64_t i = 0; i < len; ++i) sum = sum + v[i];
      const double mean = sum / (double)len;
      double var = 0.0;
      for (int64_t i = 0; i < len; ++i) var = var + (mean - v[i]) * (mean - v[i]);
      aux[2 * r] = mean; aux[2 * r + 1] = var / (double)len;
    }
  }
}

// The training rows [nd][K] of documents d0 .. d0 + nd from their topic counts cnt [nd][K]: ModifiedSimpleLDA.calcThetaEstimate
// (MSLDA:709-753), (n_dk + alpha_k) / normaliser, or calcZBar (MSLDA:647-668), n_dk / N_d with zeros for an empty document.
// ptr = doc_ptr + d0.
// sim_doc_norm_kernel: norm[d] = the normaliser, the sum over k IN INDEX ORDER of (double) n_dk + alpha_k.  64 lanes own 64
// documents; 64 topics at a time go through LDS, loaded a document's row segment at a time (contiguous) and added by the
// document's lane from its LDS row (stride 65 doubles: conflict-free), so the chain is the Java loop's and the loads coalesce.
constexpr int kSimNormDocs = 64;
__global__ __launch_bounds__(kSimNormDocs) void sim_doc_norm_kernel(const int32_t *__restrict__ cnt, const double *__restrict__ alpha, int64_t nd, int32_t K,
                                                                    double *__restrict__ norm) {
  __shared__ double t[kSimNormDocs][kSimNormDocs + 1];
  const int lane = threadIdx.x;
  const int64_t d0 = (int64_t)blockIdx.x * kSimNormDocs;
  const int rows = (int)(nd - d0 < kSimNormDocs ? nd - d0 : kSimNormDocs);
  double normalizer = 0.0;
  for (int32_t k0 = 0; k0 < K; k0 += kSimNormDocs) {
    const int kn = K - k0 < kSimNormDocs ? K - k0 : kSimNormDocs;
    if (lane < kn)
      for (int r = 0; r < rows; ++r) t[r][lane] = (double)cnt[(d0 + r) * K + k0 + lane] + alpha[k0 + lane];
    __syncthreads();
    if (lane < rows)
      for (int k = 0; k < kn; ++k) normalizer = normalizer + t[lane][k];
    __syncthreads();
  }
  if (lane < rows) norm[d0 + lane] = normalizer;
}
// one lane per cell
__global__ __launch_bounds__(256) void sim_doc_rows_kernel(const int32_t *__restrict__ cnt, const int64_t *__restrict__ ptr, const double *__restrict__ alpha,
                                                           const double *__restrict__ norm, int64_t nd, int32_t K, int zbar, double *__restrict__ rows) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nd * K; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t d = e / K;
    const int32_t k = (int32_t)(e - d * K);
    if (zbar) {
      const int64_t n = ptr[d + 1] - ptr[d];
      rows[e] = n ? (double)cnt[e] / (double)n : 0.0;
    } else {
      rows[e] = ((double)cnt[e] + alpha[k]) / norm[d];
    }
  }
}

// (d, i) into the list ld / li [n] (stride `st`) kept in the order of the header; the caller has checked d < +inf
__device__ __forceinline__ void sim_insert(double *ld, int64_t *li, int st, int n, double d, int64_t i) {
  if (!(d < ld[(n - 1) * st])) return;
  int p = n - 1;
  while (p > 0 && ld[(p - 1) * st] > d) {
    ld[p * st] = ld[(p - 1) * st]; li[p * st] = li[(p - 1) * st];
    --p;
  }
  ld[p * st] = d; li[p * st] = i;
}

struct SimParams {
  const double *A, *B;                 // [n][len], [m][len]
  const double *auxA, *auxB;           // [n][2], [m][2], or null
  const int64_t *ptrA;                 // [n + 1]: A's document r is empty when ptrA[r + 1] == ptrA[r]; null: none is
  const int64_t *lenB;                 // [m]: the queries' lengths; null: none is empty
  int64_t n, m, len;
  int64_t tiles_a, segs, tiles_per_seg;
  int64_t base_a;                      // the global index of A's row 0
  double *out;                         // dense: value (q, r) at out[q * out_pitch + r]
  int64_t out_pitch;
  double *part_d;                      // nearest: [m][segs][n_nearest]
  int64_t *part_i;
  int32_t n_nearest;                   // 0: dense
};

constexpr int sim_lds_doubles(int R) {
  // the staging buffers (reused as the [T][T + 1] tile of values: KC >= T / 2) + the lists' distances and indices
  return 2 * kSimKC * (16 * R + 1) + 2 * kSimMaxNearest * 16 * R;
}

// index k of a lane's R x R pairs: as[16 i] are its rows' staged values, bs[16 j] its partners'
template <class M>
__device__ __forceinline__ void sim_steps(typename M::Acc (&acc)[M::R][M::R], const double *as, const double *bs, int k) {
  constexpr int R = M::R;
  double a[R], b[R];
#pragma unroll
  for (int i = 0; i < R; ++i) a[i] = as[16 * i];
#pragma unroll
  for (int j = 0; j < R; ++j) b[j] = bs[16 * j];
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int j = 0; j < R; ++j) M::step(acc[i][j], a[i], b[j], k);
}

template <class M>
__global__ __launch_bounds__(kDistBlock) void sim_tile_kernel(SimParams p) {
  constexpr int R = M::R, T = 16 * R, LD = T + 1, KC = kSimKC;
  static_assert(2 * KC >= T, "the tile of values reuses the staging buffers");
  __shared__ double lds[sim_lds_doubles(R)];
  double *As = lds, *Bs = lds + KC * LD, *vals = lds;
  double *list_d = lds + 2 * KC * LD;
  int64_t *list_i = reinterpret_cast<int64_t *>(list_d + kSimMaxNearest * T);
  const int64_t qt = blockIdx.x / p.segs, seg = blockIdx.x - qt * p.segs;
  const int64_t c0 = qt * T;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int nn = p.n_nearest;
  if (nn && tid < T)
    for (int e = 0; e < nn; ++e) { list_d[e * T + tid] = sim_inf(); list_i[e * T + tid] = -1; }

  const int64_t t_end = p.tiles_per_seg * (seg + 1) < p.tiles_a ? p.tiles_per_seg * (seg + 1) : p.tiles_a;
  for (int64_t ta = p.tiles_per_seg * seg; ta < t_end; ++ta) {
    const int64_t r0 = ta * T;
    typename M::Acc acc[R][R];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
      for (int j = 0; j < R; ++j) M::init(acc[i][j]);

    for (int64_t k0 = 0; M::kLoop && k0 < p.len; k0 += KC) {
      const int kn = (int)(p.len - k0 < KC ? p.len - k0 : KC);
      for (int e = tid; e < KC * T; e += kDistBlock) {
        const int r = e / KC, kk = e - r * KC;
        if (kk < kn) {
          As[kk * LD + r] = r0 + r < p.n ? M::stage(p.A[(r0 + r) * p.len + k0 + kk], p.auxA + 2 * (r0 + r)) : 0.0;
          Bs[kk * LD + r] = c0 + r < p.m ? M::stage(p.B[(c0 + r) * p.len + k0 + kk], p.auxB + 2 * (c0 + r)) : 0.0;
        }
      }
      __syncthreads();
      if (kn == KC) {
#pragma unroll M::kUnroll
        for (int kk = 0; kk < KC; ++kk) sim_steps<M>(acc, As + kk * LD + ty, Bs + kk * LD + tx, (int)k0 + kk);
      } else {
        for (int kk = 0; kk < kn; ++kk) sim_steps<M>(acc, As + kk * LD + ty, Bs + kk * LD + tx, (int)k0 + kk);
      }
      __syncthreads();
    }

    // the tile's values as [query][document], the length rule applied
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int64_t r = r0 + ty + 16 * i;
      const bool live_a = r < p.n;
      const bool empty_a = live_a && p.ptrA && p.ptrA[r + 1] == p.ptrA[r];
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const int64_t c = c0 + tx + 16 * j;
        double v = sim_inf();
        if (live_a && c < p.m) {
          const bool empty_b = p.lenB && p.lenB[c] == 0;
          if (empty_a || empty_b) v = empty_a && empty_b ? 0.0 : sim_inf();
          else v = M::finish(acc[i][j], p.auxA + 2 * r, p.auxB + 2 * c, p.len);
        }
        vals[(tx + 16 * j) * LD + ty + 16 * i] = v;
      }
    }
    __syncthreads();
    if (nn) {
      if (tid < T && c0 + tid < p.m) {
        const int64_t rows = p.n - r0 < T ? p.n - r0 : T;
        for (int r = 0; r < (int)rows; ++r) {
          const double v = vals[tid * LD + r];
          if (v < sim_inf()) sim_insert(list_d + tid, list_i + tid, T, nn, v, p.base_a + r0 + r);
        }
      }
    } else {
      for (int e = tid; e < T * T; e += kDistBlock) {
        const int q = e / T, r = e - q * T;
        if (c0 + q < p.m && r0 + r < p.n) p.out[(c0 + q) * p.out_pitch + r0 + r] = vals[q * LD + r];
      }
    }
    __syncthreads();
  }
  if (nn && tid < T && c0 + tid < p.m) {
    const int64_t o = ((c0 + tid) * p.segs + seg) * nn;
    for (int e = 0; e < nn; ++e) { p.part_d[o + e] = list_d[e * T + tid]; p.part_i[o + e] = list_i[e * T + tid]; }
  }
}

// res [m][n] <- the n best of (res, unless `first`) and the lists part [m][segs][n]; what comes earlier has the lower indices
__global__ __launch_bounds__(kSimMergeBlock) void sim_merge_kernel(const double *__restrict__ part_d, const int64_t *__restrict__ part_i, int64_t m, int64_t segs, int n,
                                                                   int first, double *__restrict__ res_d, int64_t *__restrict__ res_i) {
  __shared__ double list_d[kSimMaxNearest * kSimMergeBlock];
  __shared__ int64_t list_i[kSimMaxNearest * kSimMergeBlock];
  const int tid = threadIdx.x;
  const int64_t q = (int64_t)blockIdx.x * kSimMergeBlock + tid;
  if (q >= m) return;                                  // no barrier below: a lane's list is its own
  for (int e = 0; e < n; ++e) {
    list_d[e * kSimMergeBlock + tid] = first ? sim_inf() : res_d[q * n + e];
    list_i[e * kSimMergeBlock + tid] = first ? -1 : res_i[q * n + e];
  }
  for (int64_t e = 0; e < segs * n; ++e) {
    const double v = part_d[q * segs * n + e];
    if (v < sim_inf()) sim_insert(list_d + tid, list_i + tid, kSimMergeBlock, n, v, part_i[q * segs * n + e]);
  }
  for (int e = 0; e < n; ++e) { res_d[q * n + e] = list_d[e * kSimMergeBlock + tid]; res_i[q * n + e] = list_i[e * kSimMergeBlock + tid]; }
}

}  // namespace ggs
