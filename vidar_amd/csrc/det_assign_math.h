// One (layer, sample) assignment problem of the detection loss tail: linear sum assignment of a [Q, G] fp32 cost block
// by shortest augmenting paths with dual variables (the textbook algorithm behind scipy.optimize.linear_sum_assignment,
// written from its description; no SciPy text is used).
//
// ONE body for the kernel and the host test.  `solve_problem` is written against a Team:
//   team.lanes()            number of lanes that share the problem
//   team.each(f)            f(lane) for every lane -- the kernel's Team calls f(threadIdx.x) in every thread, the host
//                           Team of tests/det_assign_host.cpp is a plain `for (lane = 0; lane < lanes; ++lane) f(lane)`
//   team.one(f)             f() once (kernel: thread 0)
//   team.sync()             workgroup barrier (host: nothing)
//   team.vote(lane, flag) / team.any()             workgroup OR
//   team.offer(lane, value, index) / team.argmin(&value, &index)   workgroup minimum that carries its index; two calls
//                           may follow each other with no sync() between them (the kernel's Team alternates its scratch)
// Everything outside each() / one() is uniform: every kernel thread evaluates it on the same values.
// Compile with -ffp-contract=off: the kernel and the host program then round identically and give the same bytes.
//
// Algorithm.  Rows are the SHORTER side (N = min(Q, G)), columns the longer one (M = max(Q, G)); with Q > G the rows are
// the ground truth, as SciPy transposes.  For every row a Dijkstra-like search grows a set of scanned columns: the lanes
// scan the columns that are still open (column j belongs to lane j % lanes), relax `shortest[j]` through the row that
// was reached last, and the team takes the minimum.  EQUAL MINIMA RESOLVE TO THE LOWEST COLUMN INDEX: (value, index) is
// totally ordered, so the result does not depend on lane count, wave count or arrival order.  The search ends at the
// first unassigned column; the duals are updated once per row and the path is walked back by one lane.
// Duals, path costs and the reduced costs are fp64 (the fp32 costs are widened): with fp32 duals a 900 x 512 problem
// comes out worse by 1e-6.  On a unique optimum the assignment equals SciPy's; on exact ties only the total does.
//
// Every loop carries its trip bound in its condition: N rows; at most M + 1 search steps per row (each step closes one
// more column); at most N + 1 steps of the walk back (a path visits a row once).  No input makes it spin.
//
// status: 0 solved; 1 the block holds NaN or -inf (SciPy: "matrix contains invalid numeric entries") -- found by a
// pre-pass over the whole block, the search is not entered; 2 every perfect matching of the short side needs a +inf
// entry (SciPy: "cost matrix is infeasible") -- a +inf entry is legal, so this one shows in the search, when the minimum
// over the open columns is +inf, and the search stops there; 3 the problem is larger than the state (kMaxLong /
// kMaxShort) or its gt_start range is not inside 0 .. total_g.  A problem with a non-zero status gets -1 in all of its
// `matched` row.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define VIDAR_DET_ASSIGN_FN __device__ __forceinline__
#else
#define VIDAR_DET_ASSIGN_FN inline
#endif

namespace vidar_det_assign {

// Supported extent, from the LDS the kernel declares for State (det_assign.hip): 8 (N + 2 M) + 4 (N + 2 M) + M bytes
// = 62 KiB at 1024 x 2048, plus the reduction scratch -- one workgroup, under 64 KiB.  Q = 900 against up to 2048 boxes
// of one sample fits (the largest nuScenes frame holds a few hundred).
constexpr int kMaxLong = 2048;    // M: the longer side
constexpr int kMaxShort = 1024;   // N: the shorter side
constexpr int kScan = 4;          // columns a lane handles per trip of the scan (one trip up to 2048 columns at 512 lanes)

enum Status : int32_t { kSolved = 0, kInvalid = 1, kInfeasible = 2, kExtent = 3 };

// pointers into LDS (kernel) or host vectors of exactly N resp. M elements (host test, so that the address sanitizer
// sees any index beyond the problem)
struct State {
  double* u;          // [N] row duals
  double* v;          // [M] column duals
  double* shortest;   // [M] shortest path cost to a column in the current search
  int32_t* path;      // [M] predecessor row of a column on that path
  int32_t* col4row;   // [N] matching, row -> column
  int32_t* row4col;   // [M] matching, column -> row
  uint8_t* closed;    // [M] column already scanned in the current search
};

// cost: the [Q, G] row-major block.  tcost: NULL, or room for a [G, Q] transposed copy that the pre-pass fills when
// Q > G, so that a row scan (fixed ground truth, all queries) reads consecutive addresses.  matched: [Q].
template <class Team>
VIDAR_DET_ASSIGN_FN int32_t solve_problem(Team& team, const float* cost, float* tcost, int Q, int G, State s,
                                          int32_t* matched) {
  const int L = team.lanes();
  const bool rows_are_gt = Q > G;
  const int N = rows_are_gt ? G : Q, M = rows_are_gt ? Q : G;
  if (N <= 0) {                                    // nothing to assign: every query is background
    team.each([&](int lane) {
      for (int q = lane; q < Q; q += L) matched[q] = -1;
    });
    return kSolved;
  }
  int32_t status = (M > kMaxLong || N > kMaxShort) ? kExtent : kSolved;

  // ---- pre-pass: entries SciPy rejects; the transposed copy on the way ----
  if (status == kSolved) {
    const bool copy = rows_are_gt && tcost != nullptr;
    const int dq = L / G, dg = L % G;              // e += L as a step of (q, g), without a division per entry
    team.each([&](int lane) {
      bool bad = false;
      int q = lane / G, g = lane % G;
      for (int e = lane; e < Q * G; e += L) {
        const float c = cost[e];
        bad = bad || c != c || c == -INFINITY;
        if (copy) tcost[g * Q + q] = c;
        q += dq;
        g += dg;
        if (g >= G) {
          g -= G;
          ++q;
        }
      }
      team.vote(lane, bad);
    });
    if (team.any()) status = kInvalid;             // any() is a barrier: the copy is complete behind it
  }
  // element (row i, column j) is base[i * rs + j * cs]
  const float* base = (rows_are_gt && tcost != nullptr) ? tcost : cost;
  const int rs = rows_are_gt ? (tcost != nullptr ? Q : 1) : G;
  const int cs = rows_are_gt ? (tcost != nullptr ? 1 : G) : 1;

  if (status == kSolved) {
    team.each([&](int lane) {
      for (int j = lane; j < M; j += L) {
        s.v[j] = 0.0;
        s.row4col[j] = -1;
      }
      for (int i = lane; i < N; i += L) {
        s.u[i] = 0.0;
        s.col4row[i] = -1;
      }
    });
    team.sync();
  }

  for (int cur = 0; cur < N && status == kSolved; ++cur) {
    team.each([&](int lane) {
      for (int j = lane; j < M; j += L) {
        s.shortest[j] = INFINITY;
        s.closed[j] = 0;
      }
    });
    team.sync();
    double min_val = 0.0;
    int i = cur, sink = -1;
    for (int step = 0; step <= M && sink < 0 && status == kSolved; ++step) {
      const double ui = s.u[i];
      const float* row = base + (int64_t)i * rs;
      team.each([&](int lane) {
        double best = INFINITY;
        int best_j = INT32_MAX;
        // kScan columns per trip: their cost loads are issued together (closed columns included, they are in bounds),
        // so a lane waits for the memory once per trip, not once per column
        for (int j0 = lane; j0 < M; j0 += kScan * L) {
          float c[kScan];
#pragma unroll
          for (int k = 0; k < kScan; ++k) {
            const int j = j0 + k * L;
            c[k] = j < M ? row[(int64_t)j * cs] : 0.0f;
          }
#pragma unroll
          for (int k = 0; k < kScan; ++k) {
            const int j = j0 + k * L;
            if (j >= M || s.closed[j]) continue;
            const double r = min_val + (double)c[k] - ui - s.v[j];
            double d = s.shortest[j];
            if (r < d) {
              d = r;
              s.shortest[j] = r;
              s.path[j] = i;
            }
            if (d < best) {                        // j grows inside a lane: the first of equal values stays
              best = d;
              best_j = j;
            }
          }
        }
        team.offer(lane, best, best_j);
      });
      int j = INT32_MAX;
      team.argmin(&min_val, &j);
      if (!(min_val < INFINITY) || j < 0 || j >= M) {
        status = kInfeasible;                      // only +inf is left among the open columns
      } else {
        // the column's own lane closes it: only that lane reads the flag in the scans, and row4col does not change
        // during a search, so the barrier inside argmin() is the only one a step needs
        team.each([&](int lane) {
          if (j % L == lane) s.closed[j] = 1;
        });
        const int r = s.row4col[j];
        if (r < 0) sink = j; else i = r;
      }
    }
    if (status == kSolved && sink < 0) status = kInfeasible;   // unreachable: N <= M, every step closes a new column
    if (status != kSolved) break;

    // duals: the rows reached are `cur` and the partners of the closed columns (the sink has none)
    team.each([&](int lane) {
      for (int j = lane; j < M; j += L) {
        if (!s.closed[j]) continue;
        const double d = min_val - s.shortest[j];
        const int r = s.row4col[j];
        if (r >= 0) s.u[r] += d;
        s.v[j] -= d;
      }
    });
    team.sync();                                   // the walk back rewrites row4col
    team.one([&]() {
      s.u[cur] += min_val;
      // walk the path back from the sink, flipping the matching
      int j = sink;
      for (int k = 0; k <= N && j >= 0; ++k) {
        const int r = s.path[j];
        if (r < 0 || r >= N) break;                // a closed column always has a predecessor row: never taken
        s.row4col[j] = r;
        const int next = s.col4row[r];
        s.col4row[r] = j;
        j = r == cur ? -1 : next;
      }
    });
    team.sync();
  }

  team.each([&](int lane) {
    for (int q = lane; q < Q; q += L) {
      int m = -1;
      if (status == kSolved) m = rows_are_gt ? s.row4col[q] : s.col4row[q];
      matched[q] = m;
    }
  });
  return status;
}

}  // namespace vidar_det_assign
