// K18  Girvan-Newman partition of the bond graph (-cg_method newman) -- replaces get_partition
// (CoarseGrainingVAE/datasets.py:373-385: networkx.community.girvan_newman, which recomputes all-pairs edge betweenness in
// Python after every edge removal).  One removal is three launches; nothing waits for another workgroup inside a launch.
//
//   newman_betweenness_k   grid of workgroups, each walks a fixed contiguous range of sources.  Per source: Brandes'
//                          algorithm on the live edges -- a level-synchronous BFS with a frontier queue (one barrier per
//                          level), path counts sigma pulled from the level above, then dependencies delta pulled from the
//                          level below, deepest level first.  Pull form: the thread that owns a node sums over its slots in
//                          CSR order, so no floating-point atomic exists and every value has one fixed summation order.
//                          Each (source, edge) contribution is added once, by the thread of the edge's shallower endpoint,
//                          to the workgroup's private row; sources follow each other, so a row's order is fixed too.
//                          State per workgroup: sigma, delta [n] fp64, row [m] fp64, level, queue, level offsets, row
//                          pointers [n] and the live neighbour of every slot [2m] -- in LDS (resident) or in the caller's
//                          workspace (streamed).  Same arithmetic, same order: the two forms give the same bits.
//   newman_choose_k        one workgroup: adds the partial rows in row order, takes the maximum over live edges, and among
//                          the live edges within a relative 1e-9 of it removes the one with the lowest (min(u,v), max(u,v)).
//   newman_components_k    one workgroup: BFS from one endpoint of the removed edge; when the other endpoint is not reached
//                          the component has split: both parts are relabelled with their lowest atom index and the
//                          component counter goes up.  Mode 0 labels the whole graph (one BFS per component).
// All three return at once when the counter has reached n_cgs, so a batch of removals may be enqueued blind.
#include "steploop_dev.h"

namespace cgv {

constexpr size_t NM_LDS_LIMIT = 159 * 1024;       // one workgroup may hold all of a CU's 160 KB of LDS (1 KB left to statics)
constexpr int NM_MAX_ATOMS = 1 << 20;
constexpr int NM_MAX_EDGES = 1 << 22;
constexpr int NM_MAX_GROUPS = 512;                // workgroups of the betweenness launch under the rule (two per CU)
constexpr int NM_WIDE = 1024;                     // threads of the two single-workgroup kernels
constexpr double NM_TIE = 1e-9;

struct NmLayout {                                 // byte offsets of one workgroup's state (8-byte values first)
  size_t sigma, delta, row, level, queue, lvl_off, rowp, adj, bytes;
};
__host__ __device__ inline NmLayout nm_layout(int n, int m) {
  NmLayout L;
  size_t o = 0;
  L.sigma = o, o += (size_t)n * 8;
  L.delta = o, o += (size_t)n * 8;
  L.row = o, o += (size_t)m * 8;
  L.level = o, o += (size_t)n * 4;
  L.queue = o, o += (size_t)n * 4;
  L.lvl_off = o, o += (size_t)(n + 2) * 4;
  L.rowp = o, o += (size_t)(n + 1) * 4;
  L.adj = o, o += (size_t)m * 8;
  L.bytes = (o + 255) & ~(size_t)255;
  return L;
}

inline int nm_groups(int n, int groups) {         // workgroups actually launched: equal ranges of ceil(n / groups) sources
  int g = groups > 0 ? groups : NM_MAX_GROUPS;
  g = g < n ? g : n;
  if (g < 1) g = 1;
  const int chunk = (n + g - 1) / g;
  return (n + chunk - 1) / chunk;
}
inline int nm_threads(int n) { return n <= 128 ? 64 : 256; }   // a single wave for small molecules

struct NmWorkspace {                              // the caller's workspace
  size_t partial, bet, mark, queue, state, bytes;
};
inline NmWorkspace nm_workspace(int n, int m, int form, int groups) {
  NmWorkspace W;
  const int g = nm_groups(n, groups);
  size_t o = 0;
  W.partial = o, o += (size_t)g * m * 8;
  W.bet = o, o += (size_t)m * 8;
  W.mark = o, o += (size_t)n * 4;
  W.queue = o, o += (size_t)n * 4;
  o = (o + 255) & ~(size_t)255;
  W.state = o;
  if (form == CGV_NEWMAN_STREAMED) o += (size_t)g * nm_layout(n, m).bytes;
  W.bytes = o + 256;
  return W;
}

// ---------------------------------------------------------------------------------------------------- betweenness
template <bool RESIDENT>
__global__ void __launch_bounds__(256)
newman_betweenness_k(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int32_t* __restrict__ edge_id,
                     const int32_t* __restrict__ alive, int n, int m, int chunk, const int32_t* __restrict__ state, int n_cgs,
                     double* __restrict__ partial, char* __restrict__ streamed_state) {
  if (state && state[0] >= n_cgs) return;
  extern __shared__ __attribute__((aligned(16))) char nm_lds[];
  __shared__ int cnt[3];
  const NmLayout L = nm_layout(n, m);
  char* base = RESIDENT ? nm_lds : streamed_state + (size_t)blockIdx.x * L.bytes;
  double* sigma = (double*)(base + L.sigma);
  double* delta = (double*)(base + L.delta);
  double* row = (double*)(base + L.row);
  int* level = (int*)(base + L.level);
  int* queue = (int*)(base + L.queue);
  int* lvl_off = (int*)(base + L.lvl_off);
  int* rowp = (int*)(base + L.rowp);
  int* adj = (int*)(base + L.adj);
  const int tid = threadIdx.x, T = blockDim.x;

  for (int e = tid; e < m; e += T) row[e] = 0.0;
  for (int v = tid; v <= n; v += T) rowp[v] = rowptr[v];
  for (int j = tid; j < 2 * m; j += T) adj[j] = alive[edge_id[j]] ? col[j] : -1;      // the live neighbour of slot j
  const int s0 = blockIdx.x * chunk, s1 = min(n, s0 + chunk);

  for (int s = s0; s < s1; ++s) {
    __syncthreads();                                           // the staging above / the previous source's last level
    for (int v = tid; v < n; v += T) level[v] = -1;
    if (tid == 0) cnt[0] = cnt[1] = cnt[2] = 0;
    __syncthreads();
    if (tid == 0) level[s] = 0, sigma[s] = 1.0, delta[s] = 0.0, queue[0] = s, lvl_off[0] = 0;
    __syncthreads();
    // forward: the nodes of level d are queue[lo, hi).  Each gets its path count from level d - 1 and discovers level d + 1
    // (integer compare-and-swap on the level, integer counter for the queue slot: the ORDER inside a level is free, no
    // value depends on it).  Three counters in turn: the one of level d + 1 is cleared while level d's is written and level
    // d - 1's is read, so one barrier per level is enough.
    int lo = 0, hi = 1, d = 0;
    while (lo < hi) {
      if (tid == 0) cnt[(d + 1) % 3] = 0, lvl_off[d + 1] = hi;
      for (int i = lo + tid; i < hi; i += T) {
        const int v = queue[i];
        const int j0 = rowp[v], j1 = rowp[v + 1];
        if (d > 0) {
          double acc = 0.0;
          for (int j = j0; j < j1; ++j) {
            const int w = adj[j];
            if (w >= 0 && level[w] == d - 1) acc += sigma[w];
          }
          sigma[v] = acc, delta[v] = 0.0;
        }
        for (int j = j0; j < j1; ++j) {
          const int w = adj[j];
          if (w >= 0 && level[w] == -1 && atomicCAS(&level[w], -1, d + 1) == -1) queue[hi + atomicAdd(&cnt[d % 3], 1)] = w;
        }
      }
      __syncthreads();
      lo = hi, hi += cnt[d % 3], ++d;
    }
    // d levels were filled (0 .. d - 1); lvl_off[d] = end of the queue.  backward, deepest level first: a node of level k
    // sums over its neighbours of level k + 1; each live edge between two levels is met exactly once per source, here.
    for (int k = d - 2; k >= 0; --k) {
      const int a = lvl_off[k], b = lvl_off[k + 1];
      for (int i = a + tid; i < b; i += T) {
        const int v = queue[i];
        const double sv = sigma[v];
        double acc = 0.0;
        for (int j = rowp[v], j1 = rowp[v + 1]; j < j1; ++j) {
          const int w = adj[j];
          if (w >= 0 && level[w] == k + 1) {
            const double c = sv / sigma[w] * (1.0 + delta[w]);
            acc += c;
            row[edge_id[j]] += c;
          }
        }
        delta[v] = acc;
      }
      __syncthreads();
    }
  }
  __syncthreads();
  for (int e = tid; e < m; e += T) partial[(size_t)blockIdx.x * m + e] = row[e];
}

// ---------------------------------------------------------------------------------------------------- reduce, choose, remove
__global__ void __launch_bounds__(NM_WIDE)
newman_choose_k(const double* __restrict__ partial, int rows, const int32_t* __restrict__ edges, int32_t* __restrict__ alive, int m,
                int32_t* __restrict__ state, int n_cgs, int remove, double* __restrict__ bet, int32_t* __restrict__ log) {
  if (state && state[0] >= n_cgs) return;
  __shared__ double red_d[NM_WIDE];
  __shared__ unsigned long long red_k[NM_WIDE];
  const int tid = threadIdx.x;
  double best = -1.0;
  for (int e = tid; e < m; e += NM_WIDE) {
    double acc = 0.0;
    constexpr int U = 8;                                       // rows whose loads are in flight together; added in row order
    for (int r0 = 0; r0 < rows; r0 += U) {
      double v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = partial[(size_t)min(r0 + u, rows - 1) * m + e];
#pragma unroll
      for (int u = 0; u < U; ++u) acc += (r0 + u < rows) ? v[u] : 0.0;
    }
    bet[e] = acc;
    if (alive[e]) best = fmax(best, acc);
  }
  if (!remove) return;
  red_d[tid] = best;
  __syncthreads();
  for (int s = NM_WIDE / 2; s > 0; s >>= 1) {
    if (tid < s) red_d[tid] = fmax(red_d[tid], red_d[tid + s]);
    __syncthreads();
  }
  const double top = red_d[0];
  if (top < 0.0) return;                                       // no live edge (uniform)
  const double thr = top - NM_TIE * top;
  unsigned long long key = ~0ull;                              // (min(u,v), max(u,v), edge) packed: the lowest wins
  for (int e = tid; e < m; e += NM_WIDE)
    if (alive[e] && bet[e] >= thr) {                           // bet[e]: this thread's own store above
      const unsigned u = (unsigned)min(edges[2 * e], edges[2 * e + 1]), v = (unsigned)max(edges[2 * e], edges[2 * e + 1]);
      const unsigned long long k = ((unsigned long long)u << 42) | ((unsigned long long)v << 22) | (unsigned)e;
      key = k < key ? k : key;
    }
  red_k[tid] = key;
  __syncthreads();
  for (int s = NM_WIDE / 2; s > 0; s >>= 1) {
    if (tid < s) red_k[tid] = red_k[tid] < red_k[tid + s] ? red_k[tid] : red_k[tid + s];
    __syncthreads();
  }
  if (tid == 0 && red_k[0] != ~0ull) {
    const int e = (int)(red_k[0] & ((1u << 22) - 1));
    alive[e] = 0;
    log[state[1]] = e;
    state[1] += 1;
  }
}

// ---------------------------------------------------------------------------------------------------- components
// BFS from `src` over live edges by the whole workgroup: mark[w] == -1 -> tag.  Stops early once `stop` is marked.
__device__ inline void nm_bfs(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int32_t* __restrict__ edge_id,
                              const int32_t* __restrict__ alive, int* mark, int* queue, int* cnt, int src, int tag, int stop) {
  const int tid = threadIdx.x;
  __syncthreads();
  if (tid == 0) mark[src] = tag, queue[0] = src, cnt[0] = cnt[1] = cnt[2] = 0;
  __syncthreads();
  int lo = 0, hi = 1, d = 0;
  while (lo < hi) {
    if (tid == 0) cnt[(d + 1) % 3] = 0;
    for (int i = lo + tid; i < hi; i += NM_WIDE) {
      const int v = queue[i];
      for (int j = rowptr[v], j1 = rowptr[v + 1]; j < j1; ++j) {
        const int w = col[j];
        if (alive[edge_id[j]] && mark[w] == -1 && atomicCAS(&mark[w], -1, tag) == -1) queue[hi + atomicAdd(&cnt[d % 3], 1)] = w;
      }
    }
    __syncthreads();
    lo = hi, hi += cnt[d % 3], ++d;
    if (stop >= 0) {                                           // every thread reads before any thread of the next level writes
      const int hit = mark[stop] != -1;
      __syncthreads();
      if (hit) break;
    }
  }
  __syncthreads();
}

__device__ inline int nm_block_min(int v, int* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = NM_WIDE / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = min(red[tid], red[tid + s]);
    __syncthreads();
  }
  return red[0];
}

template <bool RESIDENT>
__global__ void __launch_bounds__(NM_WIDE)
newman_components_k(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int32_t* __restrict__ edge_id,
                    const int32_t* __restrict__ edges, const int32_t* __restrict__ alive, int n, int32_t* __restrict__ labels,
                    int32_t* __restrict__ state, int n_cgs, int mode, const int32_t* __restrict__ log, int* ws_mark, int* ws_queue) {
  if (mode != 0 && state[0] >= n_cgs) return;
  extern __shared__ __attribute__((aligned(16))) char nm_lds[];
  __shared__ int cnt[3];
  __shared__ int red[NM_WIDE];
  int* mark = RESIDENT ? (int*)nm_lds : ws_mark;
  int* queue = RESIDENT ? (int*)nm_lds + n : ws_queue;
  const int tid = threadIdx.x;
  for (int v = tid; v < n; v += NM_WIDE) mark[v] = -1;
  __syncthreads();
  if (mode == 0) {                                             // label everything: ascending starts, so label = lowest atom
    int count = 0;
    for (int s = 0; s < n; ++s) {
      if (mark[s] != -1) continue;                             // uniform: nm_bfs ends on a barrier
      nm_bfs(rowptr, col, edge_id, alive, mark, queue, cnt, s, s, -1);
      ++count;
    }
    for (int v = tid; v < n; v += NM_WIDE) labels[v] = mark[v];
    if (tid == 0) state[0] = count, state[1] = 0;
    return;
  }
  if (state[1] < 1) return;
  const int e = log[state[1] - 1];                             // the edge newman_choose_k has just removed
  const int u = edges[2 * e], v = edges[2 * e + 1];
  nm_bfs(rowptr, col, edge_id, alive, mark, queue, cnt, u, 1, v);
  if (mark[v] != -1) return;                                   // still connected (uniform)
  const int old = labels[u];
  int mine = n;
  for (int w = tid; w < n; w += NM_WIDE)
    if (mark[w] != -1) mine = min(mine, w);
  const int min_a = nm_block_min(mine, red);                   // lowest atom of u's side
  if (min_a != old) {
    for (int w = tid; w < n; w += NM_WIDE)
      if (mark[w] != -1) labels[w] = min_a;
  } else {                                                     // u's side keeps the label: the rest of the old component moves
    mine = n;
    for (int w = tid; w < n; w += NM_WIDE)
      if (mark[w] == -1 && labels[w] == old) mine = min(mine, w);
    const int min_b = nm_block_min(mine, red);
    for (int w = tid; w < n; w += NM_WIDE)
      if (mark[w] == -1 && labels[w] == old) labels[w] = min_b;
  }
  if (tid == 0) state[0] += 1;
}

static int nm_resident_fits(int n, int m) { return nm_layout(n, m).bytes <= NM_LDS_LIMIT; }

static int nm_check(int n, int m, int form, const void* workspace, size_t workspace_bytes, int groups, const char* who) {
  if (n < 1 || n > NM_MAX_ATOMS || m < 0 || m > NM_MAX_EDGES) {
    set_error("%s: 1 <= n <= %d atoms and 0 <= m <= %d edges", who, NM_MAX_ATOMS, NM_MAX_EDGES);
    return CGV_E_BADARG;
  }
  if (form != CGV_NEWMAN_RESIDENT && form != CGV_NEWMAN_STREAMED) {
    set_error("%s: form must be CGV_NEWMAN_RESIDENT or CGV_NEWMAN_STREAMED", who);
    return CGV_E_BADARG;
  }
  if (form == CGV_NEWMAN_RESIDENT && !nm_resident_fits(n, m)) {
    set_error("%s: %d atoms / %d edges do not fit the resident form (cgv_newman_resident_fits)", who, n, m);
    return CGV_E_UNSUPPORTED;
  }
  if (groups < 0) {
    set_error("%s: groups >= 0", who);
    return CGV_E_BADARG;
  }
  if (!workspace || workspace_bytes < nm_workspace(n, m, form, groups).bytes || ((uintptr_t)workspace & 255)) {
    set_error("%s: workspace smaller than cgv_newman_workspace_bytes() or not 256-byte aligned", who);
    return CGV_E_BADARG;
  }
  return 0;
}

static int nm_launch_betweenness(const int32_t* rowptr, const int32_t* col, const int32_t* edge_id, const int32_t* alive, int n, int m,
                                 int form, int groups, const int32_t* state, int n_cgs, char* ws, hipStream_t st) {
  const NmWorkspace W = nm_workspace(n, m, form, groups);
  const int g = nm_groups(n, groups), chunk = (n + g - 1) / g, threads = nm_threads(n);
  double* partial = (double*)(ws + W.partial);
  if (form == CGV_NEWMAN_RESIDENT) {
    const size_t lds = nm_layout(n, m).bytes;
    if (int rc = steploop::allow_lds(newman_betweenness_k<true>, lds, "cgv_newman_betweenness")) return rc;
    hipLaunchKernelGGL(newman_betweenness_k<true>, dim3((unsigned)g), dim3(threads), lds, st, rowptr, col, edge_id, alive, n, m,
                       chunk, state, n_cgs, partial, (char*)nullptr);
  } else {
    hipLaunchKernelGGL(newman_betweenness_k<false>, dim3((unsigned)g), dim3(threads), 0, st, rowptr, col, edge_id, alive, n, m,
                       chunk, state, n_cgs, partial, ws + W.state);
  }
  return check_launch("cgv_newman (betweenness)");
}

static int nm_launch_components(const int32_t* rowptr, const int32_t* col, const int32_t* edge_id, const int32_t* edges,
                                const int32_t* alive, int n, int m, int form, int groups, int32_t* labels, int32_t* state, int n_cgs,
                                int mode, const int32_t* log, char* ws, hipStream_t st) {
  const NmWorkspace W = nm_workspace(n, m, form, groups);
  int *mark = (int*)(ws + W.mark), *queue = (int*)(ws + W.queue);
  const size_t lds = (size_t)n * 8;
  if (form == CGV_NEWMAN_RESIDENT && lds <= NM_LDS_LIMIT - 8 * 1024) {      // mark + queue beside 4 KB of statics
    if (int rc = steploop::allow_lds(newman_components_k<true>, lds, "cgv_newman_components")) return rc;
    hipLaunchKernelGGL(newman_components_k<true>, dim3(1), dim3(NM_WIDE), lds, st, rowptr, col, edge_id, edges, alive, n, labels,
                       state, n_cgs, mode, log, mark, queue);
  } else {
    hipLaunchKernelGGL(newman_components_k<false>, dim3(1), dim3(NM_WIDE), 0, st, rowptr, col, edge_id, edges, alive, n, labels,
                       state, n_cgs, mode, log, mark, queue);
  }
  return check_launch("cgv_newman (components)");
}

}  // namespace cgv

extern "C" {

int cgv_newman_resident_fits(int n, int m) {
  if (n < 1 || n > cgv::NM_MAX_ATOMS || m < 0 || m > cgv::NM_MAX_EDGES) return 0;
  return cgv::nm_resident_fits(n, m);
}

int cgv_newman_groups(int n, int groups) { return n < 1 ? 0 : cgv::nm_groups(n, groups < 0 ? 0 : groups); }

size_t cgv_newman_workspace_bytes(int n, int m, int form, int groups) {
  if (n < 1 || n > cgv::NM_MAX_ATOMS || m < 0 || m > cgv::NM_MAX_EDGES || groups < 0) return 0;
  return cgv::nm_workspace(n, m, form, groups).bytes;
}

int cgv_newman_betweenness(const int32_t* rowptr, const int32_t* col, const int32_t* edge_id, const int32_t* alive, int n, int m,
                           int form, int groups, double* bet, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = cgv::nm_check(n, m, form, workspace, workspace_bytes, groups, "cgv_newman_betweenness");
  if (rc) return rc;
  CGV_REQUIRE(rowptr && col && edge_id && alive && bet, "null pointer");
  if (m == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  rc = cgv::nm_launch_betweenness(rowptr, col, edge_id, alive, n, m, form, groups, nullptr, 0, ws, st);
  if (rc) return rc;
  const cgv::NmWorkspace W = cgv::nm_workspace(n, m, form, groups);
  hipLaunchKernelGGL(cgv::newman_choose_k, dim3(1), dim3(cgv::NM_WIDE), 0, st, (const double*)(ws + W.partial), cgv::nm_groups(n, groups),
                     (const int32_t*)nullptr, const_cast<int32_t*>(alive), m, (int32_t*)nullptr, 0, 0, bet, (int32_t*)nullptr);
  return cgv::check_launch("cgv_newman_betweenness (reduce)");
}

int cgv_newman_components(const int32_t* rowptr, const int32_t* col, const int32_t* edge_id, const int32_t* edges,
                          const int32_t* alive, int n, int m, int form, int groups, int32_t* labels, int32_t* state,
                          void* workspace, size_t workspace_bytes, void* stream) {
  int rc = cgv::nm_check(n, m, form, workspace, workspace_bytes, groups, "cgv_newman_components");
  if (rc) return rc;
  CGV_REQUIRE(rowptr && col && edge_id && edges && alive && labels && state, "null pointer");
  return cgv::nm_launch_components(rowptr, col, edge_id, edges, alive, n, m, form, groups, labels, state, 0, 0, nullptr, (char*)workspace,
                                   (hipStream_t)stream);
}

int cgv_newman_partition(const int32_t* rowptr, const int32_t* col, const int32_t* edge_id, const int32_t* edges, int32_t* alive,
                         int32_t* labels, int32_t* state, int32_t* log, int n, int m, int n_cgs, int removals, int form, int groups,
                         void* workspace, size_t workspace_bytes, void* stream) {
  int rc = cgv::nm_check(n, m, form, workspace, workspace_bytes, groups, "cgv_newman_partition");
  if (rc) return rc;
  CGV_REQUIRE(rowptr && col && edge_id && edges && alive && labels && state && log, "null pointer");
  CGV_REQUIRE(n_cgs >= 1 && n_cgs <= n, "1 <= n_cgs <= n");
  CGV_REQUIRE(removals >= 0 && removals <= m, "0 <= removals <= m");
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const cgv::NmWorkspace W = cgv::nm_workspace(n, m, form, groups);
  const int rows = cgv::nm_groups(n, groups);
  for (int r = 0; r < removals; ++r) {
    rc = cgv::nm_launch_betweenness(rowptr, col, edge_id, alive, n, m, form, groups, state, n_cgs, ws, st);
    if (rc) return rc;
    hipLaunchKernelGGL(cgv::newman_choose_k, dim3(1), dim3(cgv::NM_WIDE), 0, st, (const double*)(ws + W.partial), rows, edges, alive, m,
                       state, n_cgs, 1, (double*)(ws + W.bet), log);
    rc = cgv::check_launch("cgv_newman_partition (choose)");
    if (rc) return rc;
    rc = cgv::nm_launch_components(rowptr, col, edge_id, edges, alive, n, m, form, groups, labels, state, n_cgs, 1, log, ws, st);
    if (rc) return rc;
  }
  return 0;
}

}  // extern "C"
