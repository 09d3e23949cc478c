/*
 * cgvae_hip.h -- C ABI of libcgvae_hip.so: the MI355X (gfx950) kernels behind the
 * CoarseGrainingVAE message-passing hot path.
 *
 * The reference (wwang2/CoarseGrainingVAE) is pure Python: it has no FFI layer.  Its seam
 * for this path is (i) torch_scatter.scatter_add / scatter_mean and (ii) the forward()
 * signatures of the message blocks in CoarseGrainingVAE/conv.py.  Every entry point below
 * names the reference lines it replaces; INTEGRATION.md shows the ctypes stub a reference
 * maintainer would add to bind them.
 *
 * Conventions (all functions):
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless marked [host];
 *   - the caller owns every buffer (inputs, outputs, workspaces); the library never
 *     allocates or frees device memory and keeps no pointer after it returns;
 *   - tensors are contiguous, fp32 / int32 / int64 exactly as declared;
 *   - `stream` is a hipStream_t (NULL = default stream); launches are asynchronous and the
 *     library never synchronises the device;
 *   - return value: 0 = success; < 0 = CGV_E_* argument error; > 0 = hipError_t of a launch;
 *     cgv_last_error_string() gives a thread-local description;
 *   - re-entrant (autograd calls backward from worker threads).  The ONLY process-wide mutable state is the explicit
 *     option table below (cgv_set_option): nothing is read from the environment, and a call's result depends on its
 *     arguments and on that table alone.
 *
 * Notation: F = n_basis, R = n_rbf, E = directed edges, Nd / Ns = destination / source
 * node counts (equal for the atom and bead graphs; Nd = beads, Ns = atoms for the
 * atom->bead contraction).
 *
 * Edge geometry record ("geom"), one per edge, stride cgv_geom_stride(R) floats:
 *   [0..R)   a_n   = rbf_n(d) * env(d)          modules.py:148-172, 52-58
 *   [R]      env   = 0.5 (cos(pi d / cut) + 1)  (0 for d >= cut)
 *   [U..U+6) ux,uy,uz,ux,uy,uz with U = cgv_geom_unit_offset(R) (even); unit = r / d,
 *            d = sqrt(sum_k (r_k^2 + 1e-8))  conv.py:25-29.  Stored twice so that every adjacent
 *            pair is an aligned 64-bit scalar operand for the packed-fp32 kernels.
 * so that the distance filter of modules.py:192-197 is
 *   w[c] = sum_n Wd[c][n] * a_n + bd[c] * env.
 */
#ifndef CGVAE_HIP_H
#define CGVAE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGV_VERSION 101 /* 0.1.1: option numbering changed (18 options) */

#define CGV_E_BADARG (-1)      /* null pointer / negative size */
#define CGV_E_UNSUPPORTED (-2) /* e.g. n_rbf outside the compiled set */
#define CGV_E_WORKSPACE (-3)   /* workspace too small */

int cgv_version(void);
const char* cgv_last_error_string(void);

/* ---------------------------------------------------------------------------------------
 * Option table: A/B switches of the launchers (no reference counterpart -- the reference has no kernels to choose
 * between).  Every option has a fixed default under which the library behaves as documented per entry point; the
 * alternatives exist for measurements and for the parity tests that cover the non-default kernels.
 * Thread semantics: the table is process wide; cgv_set_option is an atomic store, every launcher reads the options it
 * uses once (relaxed atomic load) at the top of the call.  Set options before issuing the launches they should
 * affect; concurrent launches from other threads see either the old or the new value.  Values do not change WHAT is
 * computed, only which kernel computes it (summation order may differ within the documented tolerance).
 * ------------------------------------------------------------------------------------- */
enum {
  CGV_OPT_MSG_FWD_SPLIT = 0,   /* cgv_equi_msg_fwd: 4 waves share a receiver's segment: -1 auto (>= 16 edges/receiver), 0, 1 */
  CGV_OPT_MSG_BWD_SPLIT = 1,   /* cgv_equi_msg_bwd: waves split a source's segment: -1 auto (>= 48 edges/source), 0, 1 */
  CGV_OPT_CSR_BUILD = 2,       /* cgv_csr_build: 0 by rows (default), 1 two-radix-pass construction */
  CGV_OPT_PSEUDO_CHUNKS = 3,   /* cgv_pseudo_msg_bwd: cap on node chunks, 0 = built-in rule */
  CGV_OPT_WGRAD_TILING = 4,    /* cgv_wgrad_plan: 0 balanced column tiles (default), 1 widest tile */
  CGV_OPT_TILE_FWD_LDS_MIN = 5,/* cgv_tile_linear_fwd: minimum 64x64 tile count for the LDS-staged kernels (default 448); 1 = the one-slab
                                  kernel always, 3 = the three-slab ring kernel wherever it is compiled (K = 577..608, 1185..1216) */
  CGV_OPT_BWD_INPUT_WAVES = 6, /* cgv_tile_linear_bwd_input*: waves per block, 0 = built-in rule */
  CGV_OPT_PSEUDO_FWD = 7,      /* cgv_pseudo_msg_fwd*: 0 built-in rule; 1..6 = (edges in flight, records staged in LDS) variants; cgv_pseudo_msg_bwd on dense bead graphs: 4 = 8 edges in flight, 5 = records not staged in LDS */
  CGV_OPT_DECODER_FAT = 8,     /* cgv_decoder_{gate,dense,uv}_bwd: 1 (default) 8-channel blocks where the width allows, 0 always 4 */
  CGV_OPT_DECODER_WLDS = 9,    /* cgv_decoder_msg_fwd: 1 (default) weight rows by LDS-DMA when they fit in LDS, 0 register path */
  CGV_OPT_SKINNY_ROWS = 10,    /* cgv_skinny_linear_fwd: row blocks (of 16) per thread block; 0 = built-in rule, 1..4 */
  CGV_OPT_TILE_FWD_BAL = 11,   /* cgv_tile_linear_fwd: 1 (default) layers of >= 1200 outputs with more than one 32 x 32 tile per CU run as ONE larger register tile per CU where a compiled tile fits (XCD-aware tile order), 0 off, 2 every shape (tests / A-B) */
  CGV_OPT_OPTIM_ONE_LAUNCH = 12, /* cgv_optim_prepare*: 0 (default) norm pass, then the decision launch; 1 both in ONE launch (the last block decides) -- measured SLOWER on the chignolin step (1.774 against 1.763 ms): 1620 blocks arriving at one device-scope ticket cost more (~12 ns each) than the launch boundary saved; 2: as 0, and cgv_wgrad_gram keeps its separate reduce launch too (A/B: by default the LAST of a problem's eight slice blocks sums them) */
  CGV_OPT_DECODER_COLSPLIT = 13, /* cgv_decoder_{gate,dense,uv}_bwd: the column tiles of a channel group's backward-input product are split over
                                  several blocks (= CUs; grid y): these products are bound by the fp32 MFMA pipe of ONE CU -- each part repeats the
                                  prologue and writes its own columns of the group's slice.  0 one block per channel group, 1 two, 2 (default) two,
                                  three for uv_bwd (48-row tiles), 3 three everywhere */
  CGV_OPT_DECODER_NODESPLIT = 14, /* cgv_decoder_uv_fwd (and uv_bwd, see there): 1 (default) 8-channel blocks by node groups of <= 5 nodes (grid y) --
                                   a third of the MFMAs and of the x rows per block; 0 one 4-channel block over all 3 n rows */
  CGV_OPT_BWD_INPUT_SPLIT = 15, /* cgv_tile_linear_bwd_input*: few output tiles and a long reduction: -1 (default) 2 - 4 blocks per tile
                                   when a workspace is registered (cgv_tile_bwd_input_split), 1 never, 2..4 that many */
  CGV_OPT_MSG_BWD_MFMA = 16,    /* cgv_equi_msg_bwd*, scalar-only upstream: the matrix-core kernel (4 edges per fp32 MFMA, records and
                                   rows through vector loads) -1 (default) from 200 edges per node on, 1 wherever it applies
                                   (>= 48 edges per node, n_rbf <= 15, n_feat % 4 == 0), 0 never (the packed-FMA walk) */
  CGV_OPT_STREAMK = 17,         /* cgv_tile_linear_fwd / cgv_tile_*bwd_input* (and their pair / two-source forms): the LDS-staged stream-K
                                   kernel (csrc/streamk_gemm.hip: 128 x 128 tiles, the (tile, 32-deep slab) units of a launch cut into equal
                                   ranges, one block per CU; needs the workspace of cgv_tile_bwd_input_split).  0 (default) where it
                                   wins: single launches of >= 1536 rows with <= 640 outputs over a >= 1200-deep reduction (see
                                   tile_gemm.hip: sk_wanted); 1 never; 2 / 3 wherever the operands allow, with one / two blocks per CU
                                   (tests, A-B); >= 16: a grid of exactly that many blocks (experiments) */
  CGV_OPT_COUNT = 18
};
/* Measurement: store the GPU wall clock (cgv_timestamp_hz ticks per second) into *slot, in stream order; capturable. */
int cgv_timestamp(uint64_t* slot /*device*/, void* stream);
int cgv_timestamp_hz(void);
/* Measurement: the shader clock sustained under packed fp32 FMAs on `blocks` x 4 waves: out[0] = shader cycles, out[1] =
 * wall-clock ticks of one wave's span of iters x 32 FMAs (the fused message forward's peak is quoted at 2.4 GHz; it runs at this). */
int cgv_sustained_clock_probe(uint64_t* out /*device [2]*/, float* sink /*device [1]*/, int blocks, int iters, void* stream);
int cgv_set_option(int option, int value);   /* 0, or CGV_E_BADARG for an unknown option */
int cgv_get_option(int option);              /* current value (INT32_MIN for an unknown option) */
int cgv_reset_options(void);                 /* every option back to its default */

/* n_rbf values with a compiled kernel: returns 1 if supported. */
int cgv_rbf_supported(int n_rbf);
/* floats per edge-geometry record for this n_rbf, and the offset of its unit-vector block. */
int cgv_geom_stride(int n_rbf);
int cgv_geom_unit_offset(int n_rbf);

/* ---------------------------------------------------------------------------------------
 * K0  radius graph -- replaces get_neighbor_list, CoarseGrainingVAE/data.py:65-82, batched
 * over frames (the Python loop of data.py:207-252).  Pair (i,j) of one frame is an edge iff
 *   s = (dx*dx + dy*dy) + dz*dz  <=  s_star          (no FMA contraction, fp32)
 * where s_star is the largest fp32 whose host sqrt is <= cutoff (computed by the caller with
 * the host's own sqrt, see graph.py) -- this makes membership bit-identical to the reference's
 * `sqrt(s) <= cutoff` without depending on the device sqrt.  Output order is the reference's
 * (torch.nonzero, row-major: i ascending, then j ascending), node ids are batch-global like
 * CG_collate produces (data.py:262-270).  undirected != 0 keeps j > i only (data.py:79-80).
 * Two calls because the edge count is data dependent:
 *   1. cgv_radius_graph_count -> counts[n_nodes] and offsets[n_nodes+1] (exclusive scan;
 *      offsets[n_nodes] = E).  The caller reads E back and allocates.
 *   2. cgv_radius_graph_emit  -> nbr_out[E][2] int64.
 * ------------------------------------------------------------------------------------- */
int cgv_radius_graph_count(const float* xyz /*[n_nodes,3]*/, const int32_t* frame_ptr /*[n_frames+1]*/,
                           int n_frames, int n_nodes, float s_star, int undirected,
                           int32_t* counts /*[n_nodes]*/, int32_t* offsets /*[n_nodes+1]*/, void* stream);
int cgv_radius_graph_emit(const float* xyz, const int32_t* frame_ptr, int n_frames, int n_nodes, float s_star,
                          int undirected, const int32_t* offsets /*[n_nodes+1]*/, int64_t* nbr_out /*[E,2]*/,
                          void* stream);

/* ---------------------------------------------------------------------------------------
 * K7  CSR plan of a directed edge list.  The reference scatters with an UNSORTED index
 * (nbrs[:,0] after make_directed, conv.py:10-20,553-561); the kernels here reduce over
 * destination-sorted segments instead (no atomics, deterministic).  Builds, with a stable
 * sort (ties keep the original edge order):
 *   dst-sorted view : rowptr_d[Nd+1], eid_d[E] (original edge id), dst_d[E], src_d[E]
 *   src-sorted view : rowptr_s[Ns+1], eid_s[E], dst_s[E], src_s[E]      (for backward)
 * dst/src are int64 arrays read with element stride `stride` (nbrs[E,2]: dst=nbrs,
 * src=nbrs+1, stride=2).  src == NULL means src[e] = e (atom->bead contraction with
 * dst = CG_mapping, conv.py:725-731).
 * Construction: by rows -- count, scan, drop, one block per row ranks its unique (partner, edge id) keys: 5 launches per
 * view -- when the workspace (size it with cgv_csr_workspace_bytes(max(E, Nd, Ns) + 1)) has room for the row counters;
 * otherwise two stable radix passes per view.  Both give the same arrays.
 * ------------------------------------------------------------------------------------- */
size_t cgv_csr_workspace_bytes(int n_edges);
int cgv_csr_build(const int64_t* dst, const int64_t* src, int stride, int n_edges, int n_dst, int n_src,
                  int32_t* rowptr_d, int32_t* eid_d, int32_t* dst_d, int32_t* src_d,
                  int32_t* rowptr_s, int32_t* eid_s, int32_t* dst_s, int32_t* src_s,
                  void* workspace, size_t workspace_bytes, void* stream);
/* K7b  receiver-group order of the dst-sorted view, for the shared-source forward (cgv_equi_msg_fwd_grouped):
 * rb consecutive receivers form a group; the group's edges (one contiguous range of the dst-sorted view, so
 * rowptr_d still delimits it) are re-ordered by (source, receiver).  Outputs, all [E] in group order:
 *   dst_g, src_g  receiver / source of the edge      pos_g  its position in the dst-sorted view
 *   meta_g [E,2]  { slot | head << 8 | last << 9 | mask << 16 , source of the group's NEXT step }: slot = receiver - group
 *                 base; a step = a maximal run of edges of one (group, source) pair with strictly increasing receivers
 *                 (a duplicated edge opens a new step); mask = the step's slots; head = first edge of the step; last =
 *                 the step is its group's last one (it names its own source as the next).
 * One launch: a block per group ranks the group's edges by (source, receiver, position) -- at most 2 x degree keys,
 * in LDS up to 4096 per group.  Edge records for this order come from cgv_edge_geometry_grouped (below), which folds
 * meta_g into them. */
size_t cgv_group_plan_workspace_bytes(int n_edges);
int cgv_group_plan_build(const int32_t* rowptr_d /*[Nd+1]*/, const int32_t* dst_d, const int32_t* src_d, int n_edges,
                         int n_dst, int n_src, int rb, int32_t* dst_g, int32_t* src_g, int32_t* pos_g,
                         int32_t* meta_g /*[E,2]*/, void* workspace, size_t workspace_bytes, void* stream);
/* The same order from two stable radix passes over all edges (~20 launches against one): kept as the independent
 * construction the tests compare with. */
size_t cgv_group_plan_radix_workspace_bytes(int n_edges);
int cgv_group_plan_build_radix(const int32_t* dst_d, const int32_t* src_d, int n_edges, int n_dst, int n_src, int rb,
                               int32_t* dst_g, int32_t* src_g, int32_t* pos_g /*or NULL*/, int32_t* meta_g /*[E,2]*/,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * K6  edge geometry -- replaces preprocess_r (conv.py:25-29), PainnRadialBasis
 * (modules.py:148-172) and CosineEnvelope (modules.py:52-58), computed ONCE per graph and
 * cutoff and shared by every layer (the reference recomputes it in each block).
 * For sorted position p:  r = r_edges[eid[p]]                      if r_edges != NULL
 *                         r = pos_src[src[p]] - pos_dst[dst[p]]    otherwise
 * coef[n] = (n+1)*pi/cutoff and pi_f = (float)pi exactly as the host computes them.
 * ------------------------------------------------------------------------------------- */
int cgv_edge_geometry(const float* r_edges /*[E,3] or NULL*/, const int32_t* eid /*[E]*/,
                      const float* pos_dst /*[Nd,3]*/, const float* pos_src /*[Ns,3]*/,
                      const int32_t* dst /*[E]*/, const int32_t* src /*[E]*/, int n_edges, int n_rbf,
                      float cutoff, const float* coef /*[R]*/, float* geom /*[E,stride]*/, void* stream);
/* Records of the receiver-group order (K7b), meta words folded in; even n_rbf; stride cgv_geom_group_stride(R) floats:
 *   [0,R) a_n ; [R] env ; [R+1] meta.x (int bits) ; [R+2,R+5) ux,uy,uz ; [R+5] meta.y (int bits) ; zero padding
 * (n_rbf = 10: 16 floats = one aligned 64-byte scalar load per edge).  Same fp32 expressions as cgv_edge_geometry. */
int cgv_geom_group_stride(int n_rbf);
int cgv_geom_group_unit_offset(int n_rbf);
int cgv_edge_geometry_grouped(const float* pos_dst /*[Nd,3]*/, const float* pos_src /*[Ns,3]*/, const int32_t* dst_g,
                              const int32_t* src_g, const int32_t* meta_g /*[E,2]*/, int n_edges, int n_rbf,
                              float cutoff, const float* coef /*[R]*/, float* geom_g /*[E,group stride]*/, void* stream);

/* ---------------------------------------------------------------------------------------
 * K1  segment reduction -- replaces torch_scatter.scatter_add / scatter_mean (requirements.txt:18;
 * call sites cgvae.py:297-298,479; conv.py:553-561 when used unfused).
 *   out[s, :] = sum_{p in [rowptr[s], rowptr[s+1])} src[perm ? perm[p] : p, :]   (/ max(len,1) if mean)
 * `src` is [n_rows, C]; perm (eid_d of the CSR plan) handles an unsorted index.
 * ------------------------------------------------------------------------------------- */
int cgv_segment_reduce(const float* src, const int32_t* rowptr, const int32_t* perm, int n_seg, int channels,
                       int mean, float* out /*[n_seg,C]*/, void* stream);
/* Two reductions over one index in one launch: the encoder's H = scatter_mean(h), V = scatter_mean(v) (cgvae.py:297-298). */
int cgv_segment_reduce2(const float* src_a, int channels_a, float* out_a, const float* src_b, int channels_b, float* out_b,
                        const int32_t* rowptr, const int32_t* perm, int n_seg, int mean, void* stream);
/* backward of the above: gsrc[perm?perm[p]:p, :] = gout[seg(p), :] (* 1/max(len,1) if mean) */
int cgv_segment_broadcast(const float* gout, const int32_t* rowptr, const int32_t* perm, int n_seg, int channels,
                          int mean, float* gsrc /*[n_rows,C]*/, void* stream);
/* The two heads of a (mu, sigma) pair -- nn.Sequential(Linear, act, Linear) each, cgvae.py:366-371 / run_ala.py:184-189,
 * applied to the same features (cgvae.py:500-503, 226-229) -- as PAIRS of launches: layer j of both heads in one launch
 * (two Dense layers of one shape; x0 may equal x1), forward and backward-input, instead of one launch (forward) or two
 * (backward: row-split product + reduction) per layer.  Rows <= 16 (forward) / 64 (backward).  With gx1 == NULL the
 * backward returns the SUM of both products in gx0 (both layers read the same input: autograd's accumulation add is
 * part of the reduction launch).  ws: 2 x cgv_skinny_bwd_input_workspace_bytes(M, N, K). */
int cgv_pair_linear_fwd(const float* x0, const float* x1, const float* W0, const float* W1, const float* bias0,
                        const float* bias1, float* y0, float* y1, float* z0, float* z1, int act0, int act1, int n_rows, int N,
                        int K, void* stream);
int cgv_pair_linear_bwd_input(const float* gy0, const float* gy1, const float* z0, const float* z1, const float* W0,
                              const float* W1, int act0, int act1, float* gx0, float* gx1, int M, int N, int K, void* ws,
                              size_t ws_bytes, void* stream);
/* The same for up to cgv_multi_linear_max() = 4 layers of one shape per launch -- the prior's (mu, sigma) heads
 * (cgvae.py:398-401) and the encoder's (cgvae.py:500-503) are independent of each other too: layer j of all four heads in
 * one launch.  Tables are HOST arrays of n device pointers (read at call time).  bwd_input: ``group`` = 1 gives n outputs
 * gx[j]; ``group`` = 2 sums the products of problems 2o, 2o + 1 (two layers that read one input) into gx[o].
 * ws: n x max(cgv_skinny_bwd_input_workspace_bytes(M, N, K), 4 M K) bytes. */
int cgv_multi_linear_max(void);
int cgv_multi_linear_fwd(int n, const float* const* x, const float* const* W, const float* const* bias, float* const* y,
                         float* const* z, const int* act, int n_rows, int N, int K, void* stream);
int cgv_multi_linear_bwd_input(int n, int group, const float* const* gy, const float* const* z, const float* const* W,
                               const int* act, float* const* gx, int M, int N, int K, void* ws, size_t ws_bytes, void* stream);
/* CGequiVAE.reparametrize (cgvae.py:445-449: eps = randn_like(sigma); z = mu + eps * sigma) with the noise drawn in the
 * launch: z = mu + sigma * eps, eps ~ N(0, 1) from Philox4x32-10 + Box-Muller, stored (the backward pass needs it:
 * dz/dsigma = eps).  rng: 3 x uint64 in device memory {seed, draw number, 0}; the launch advances the draw number, so a
 * replayed hipGraph draws fresh noise each step.  Same distribution as torch.randn_like, different numbers: runs that
 * must reproduce a given eps pass it in and do not call this. */
int cgv_reparam_sample(const float* mu, const float* sigma, float* eps, float* z, int64_t n, uint64_t* rng, void* stream);
/* Its backward with the KL term's gradients (cgv_elbo_fwd's g_mu / g_sigma: the other consumer of mu and sigma,
 * scripts/utils.py:121) folded in: g_mu = g + k_mu, g_sigma = g * eps + k_sigma; n % 4 == 0. */
int cgv_reparam_bwd(const float* g, const float* eps, const float* k_mu, const float* k_sigma, float* g_mu, float* g_sigma,
                    int64_t n, void* stream);
/* nn.Embedding lookup (cgvae.py:268, 381) with the ids read from a float column (nxyz[:, 0], element stride id_stride):
 * out[i, :] = weight[(int) ids[i * id_stride], :]; ids are clamped to [0, n_types). */
int cgv_embedding_rows(const float* weight /*[n_types,C]*/, const float* ids_f32, int id_stride, int n_rows, int n_types,
                       int channels, float* out /*[n_rows,C]*/, void* stream);
/* The two embedding lookups of a step (encoder: atom types, cgvae.py:268; prior: bead types, cgvae.py:381) in one launch,
 * and their weight gradients (two segment sums over the type-id plans) in one launch. */
int cgv_embedding_rows2(const float* weight_a, const float* ids_a, int id_stride_a, int n_rows_a, int n_types_a, float* out_a,
                        const float* weight_b, const float* ids_b, int id_stride_b, int n_rows_b, int n_types_b, float* out_b,
                        int channels, void* stream);
int cgv_segment_reduce_pair(const float* src_a, const int32_t* rowptr_a, const int32_t* perm_a, int n_seg_a, float* out_a,
                            const float* src_b, const int32_t* rowptr_b, const int32_t* perm_b, int n_seg_b, float* out_b,
                            int channels, void* stream);

/* ---------------------------------------------------------------------------------------
 * K2 / K4  fused EquiMessageBlock (conv.py:505-563 incl. InvariantMessage 63-75 and
 * DistanceEmbed modules.py:192-197) and, with the atom->bead plan, ContractiveMessageBlock
 * (conv.py:703-733).  phi = inv_dense(s) is computed by the caller (node-level GEMMs).
 *   m_k(e,f) = phi[src(e), kF+f] * w[kF+f](e)
 *   ds[i,f]   = sum_{e: dst(e)=i} m_1
 *   dv[i,f,:] = sum_e ( m_2 * unit_e + m_0 * v[src(e), f, :] )
 * No [E, .] tensor is ever written.  with_dv = 0 skips the vector channel (explicit option;
 * the encoder never consumes it -- SURVEY 8a note a12) and leaves dv untouched.
 * s_res / v_res (optional): the outputs become s_res + ds and v_res + dv, i.e. the residual adds
 * of cgvae.py:287-288, 309-310, 391-392 fused into the store.
 * n_rows_hint = number of rows of the gathered arrays (Ns forward, Nd backward; 0 = unknown): enables
 * the buffer-descriptor gather path when every row lies within 2 GiB of its base.
 * n_edges_hint (the edge count, or 0) only selects the launch shape: several waves share a
 * receiver when the average degree is high.  Results do not depend on it beyond fp32
 * summation order.
 * ------------------------------------------------------------------------------------- */
int cgv_equi_msg_fwd(const float* phi /*[Ns,3F]*/, const float* v /*[Ns,F,3]*/, const float* geom_d,
                     const int32_t* rowptr_d, const int32_t* src_d, const float* Wd /*[3F,R]*/,
                     const float* bd /*[3F]*/, float* ds /*[Nd,F]*/, float* dv /*[Nd,F,3]*/, int n_dst,
                     int n_feat, int n_rbf, int with_dv, int64_t n_edges_hint, int64_t n_rows_hint,
                     const float* s_res /*[Nd,F] or NULL*/, const float* v_res /*[Nd,F,3] or NULL*/, void* stream);
/* The same forward (with the vector channel) as a shared-source walk over the receiver-group order
 * (cgv_group_plan_build with the same rb; geom_g = cgv_edge_geometry_grouped records of that order): a wave keeps rb
 * accumulator sets and gathers every source row once per group instead of once per edge -- for graphs whose consecutive receivers share
 * most of their neighbours (molecules: always).  Needs even n_feat / n_rbf, rb in {2, 4}, 8-byte aligned operands
 * (Wd, geom_g 16-byte), all n_rows rows of phi / v within 2 GiB.  Same results up to fp32 summation order. */
int cgv_equi_msg_grouped_supported(int n_feat, int n_rbf, int rb);
int cgv_equi_msg_fwd_grouped(const float* phi /*[Ns,3F]*/, const float* v /*[Ns,F,3]*/, const float* geom_g,
                             const int32_t* rowptr_d, const int32_t* src_g,
                             const float* Wd /*[3F,R]*/, const float* bd /*[3F]*/, float* ds /*[Nd,F]*/,
                             float* dv /*[Nd,F,3]*/, int n_dst, int n_feat, int n_rbf, int rb, int64_t n_rows,
                             int64_t n_edges /* records in geom_g */, const float* s_res /*[Nd,F] or NULL*/, const float* v_res /*[Nd,F,3] or NULL*/,
                             void* stream);
/* Removed after losing their A/B against the launch above (commit 028bd3e last held them; DESIGN.md 8,
 * profiles/r05_k2_parts_ab.txt, profiles/r05_k2e_*): 2-4 blocks per (group, channel tile) whose sums met in a workspace
 * (level or slower on all three workloads), the walk cut into equal edge ranges on a resident grid (chignolin 45.6
 * against 42.7 us, 2000 atoms 678 against 600), 8-wave blocks (942 against 654 us), the record stream through an LDS ring,
 * and a matrix-core filter evaluation in cgv_equi_msg_fwd (71 against 55 us). */
/* Backward.  gs / gv are the upstream gradients at the receivers (gv == NULL when dv is not
 * consumed).  Traverses the src-sorted view; writes g_phi [Ns,3F], g_v [Ns,F,3] (only if gv),
 * gWd [3F,R], gbd [3F] completely (zeros where nothing flows).  Deterministic two-stage
 * reduction for gWd/gbd through `workspace`. */
size_t cgv_equi_msg_bwd_workspace_bytes(int n_src, int n_feat, int n_rbf);
int cgv_equi_msg_bwd(const float* phi, const float* v, const float* geom_s, const int32_t* rowptr_s,
                     const int32_t* dst_s, const float* Wd, const float* bd, const float* gs /*[Nd,F] or NULL*/,
                     const float* gv /*[Nd,F,3] or NULL*/, float* g_phi, float* g_v, float* gWd, float* gbd,
                     int n_src, int n_feat, int n_rbf, int64_t n_edges_hint, int64_t n_rows_hint, void* workspace,
                     size_t workspace_bytes, void* stream);
/* The same without its second stage, for a training step that wants the filter gradients only at its end: g_phi / g_v
 * are final, gWd / gbd stay as per-chunk partial sums in `workspace` (keep it alive) and are finished -- for up to
 * cgv_filter_reduce_jobs_max() such launches at once -- by cgv_filter_reduce_jobs.  jobs_host: records
 * {const float* part; float* gWd; float* gbd; int n_chunks, K, R, F;} with part = the launch's workspace, n_chunks /
 * K = what it returned in *n_chunks / *k_live, R = n_rbf, F = n_feat.  (The filter gradients feed the optimiser only:
 * their seven reduction launches per chignolin step were seven links in the backward chain.) */
int cgv_equi_msg_bwd_deferred(const float* phi, const float* v, const float* geom_s, const int32_t* rowptr_s,
                              const int32_t* dst_s, const float* Wd, const float* bd, const float* gs, const float* gv,
                              float* g_phi, float* g_v, int n_src, int n_feat, int n_rbf, int64_t n_edges_hint,
                              int64_t n_rows_hint, void* workspace, size_t workspace_bytes, int* n_chunks, int* k_live,
                              void* stream);
int cgv_filter_reduce_jobs_max(void);
int cgv_filter_reduce_job_bytes(void);
int cgv_filter_reduce_jobs(const void* jobs_host, int n_jobs, void* stream);

/* ---------------------------------------------------------------------------------------
 * Per-batch graph work over job tables (csrc/batch_plans.hip): what cgv_csr_build and cgv_edge_geometry[_grouped] do,
 * for ALL sorted views / record arrays of a batch in 4 + 1 launches (replaces make_directed's consumers and the
 * per-block preprocess_r / rbf / envelope of conv.py:10-29, modules.py:148-197 for a whole batch at once).
 * jobs_host [host]: n records with the layout of cgv::PlanJob / cgv::GeomJob (csrc/batch_plans.hip; sizes from
 * cgv_plan_job_bytes / cgv_geom_job_bytes), device pointers inside, copied into the kernel arguments by value.
 * PlanJob.count must be ZERO on entry ([n_rows + 1] ints) and is zero again on exit.
 * ------------------------------------------------------------------------------------- */
/* Rows [n][4] = (type id, x, y, z) of a prepared batch's atoms and beads into the captured step's tensors and, as
 * contiguous [n][3] coordinates, into the graph bundle: one launch (replaces the reference DataLoader's hand-over of the
 * next batch, cgvae.py:486 / scripts/utils.py:131). */
int cgv_batch_load_rows(const float* src_atoms, float* dst_atoms, float* xyz_atoms, int n_atoms, const float* src_beads,
                        float* dst_beads, float* xyz_beads, int n_beads, void* stream);
int cgv_plan_jobs_max(void);
int cgv_plan_job_bytes(void);
int cgv_plan_jobs_build(const void* jobs_host, int n_jobs, void* stream);
int cgv_geom_jobs_max(void);
int cgv_geom_job_bytes(void);
int cgv_geom_jobs_build(const void* jobs_host, int n_jobs, void* stream);

/* ---------------------------------------------------------------------------------------
 * K3  fused EquiMessagePsuedo (conv.py:180-242), i = dst (receiver), j = src, q_k = phi[j,kF+f] w_k
 * with k = 0..8 (phi is [N,9F]), u = unit_e:
 *   dh    = sum q0 s_i                 dhbar = sum (v_i . vbar_j)      (no filter, conv.py:206)
 *   dv    = sum q1 u + q2 v_j + q3 (v_i x vbar_j) + q4 sbar_i vbar_j
 *   dvbar = sum q5 vbar_j + q6 sbar_i v_j + q7 (v_i x v_j) + q8 (vbar_i x vbar_j)
 * Backward needs both CSR views (receiver-side sums on the dst-sorted one, source-side sums,
 * g_phi and the filter gradients on the src-sorted one); any upstream gradient may be NULL.
 * All outputs are written completely.  Derivation: csrc/pseudo_msg.hip.
 * residual != 0: the outputs are the UPDATED states s + dh, sbar + dhbar, v + dv, vbar + dvbar
 * (the residual adds of cgvae.py:108-111 fused in), and the backward adds the pass-through term.
 * ------------------------------------------------------------------------------------- */
int cgv_pseudo_msg_fwd(const float* phi /*[N,9F]*/, const float* s, const float* sbar, const float* v,
                       const float* vbar, const float* geom_d, const int32_t* rowptr_d, const int32_t* src_d,
                       const float* Wd /*[9F,R]*/, const float* bd /*[9F]*/, float* dh, float* dhbar, float* dv,
                       float* dvbar, int n_nodes, int n_feat, int n_rbf, int residual, void* stream);
/* The same launch; dv_rows (or NULL) [3 N, F] additionally receives dv as rows 3 i + xyz, the operand layout of
 * UpdateBlock's u_mat / v_mat products (conv.py:591) -- saves the transpose launch in front of every decoder update. */
int cgv_pseudo_msg_fwd_rows(const float* phi, const float* s, const float* sbar, const float* v, const float* vbar,
                            const float* geom_d, const int32_t* rowptr_d, const int32_t* src_d, const float* Wd,
                            const float* bd, float* dh, float* dhbar, float* dv, float* dvbar, float* dv_rows,
                            int n_nodes, int n_feat, int n_rbf, int residual, int64_t n_edges_hint /*0: unknown; dispatch only*/,
                            void* stream);
size_t cgv_pseudo_msg_bwd_workspace_bytes(int n_nodes, int n_feat, int n_rbf);
int cgv_pseudo_msg_bwd(const float* phi, const float* s, const float* sbar, const float* v, const float* vbar,
                       const float* geom_d, const int32_t* rowptr_d, const int32_t* src_d,
                       const float* geom_s, const int32_t* rowptr_s, const int32_t* dst_s,
                       const float* Wd, const float* bd,
                       const float* gh, const float* ghbar, const float* gv, const float* gvbar,
                       float* g_phi /*[N,9F]*/, float* g_s, float* g_sbar, float* g_v, float* g_vbar,
                       float* gWd /*[9F,R]*/, float* gbd /*[9F]*/, int n_nodes, int n_feat, int n_rbf,
                       int residual, int64_t n_edges_hint /*0: unknown; dispatch only*/, void* workspace,
                       size_t workspace_bytes, void* stream);
/* cgv_pseudo_msg_bwd without its last launch (the filter-gradient reduction over chunks): the partial sums stay in
 * `workspace`; one cgv_filter_reduce_jobs launch (job K = 9, *n_chunks) finishes them together with the step's other
 * message blocks.  Replaces the same autograd as cgv_pseudo_msg_bwd (conv.py:180-242). */
int cgv_pseudo_msg_bwd_deferred(const float* phi, const float* s, const float* sbar, const float* v, const float* vbar,
                                const float* geom_d, const int32_t* rowptr_d, const int32_t* src_d, const float* geom_s,
                                const int32_t* rowptr_s, const int32_t* dst_s, const float* Wd, const float* bd, const float* gh,
                                const float* ghbar, const float* gv, const float* gvbar, float* g_phi, float* g_s, float* g_sbar,
                                float* g_v, float* g_vbar, int n_nodes, int n_feat, int n_rbf, int residual,
                                int64_t n_edges_hint, void* workspace, size_t workspace_bytes, int* n_chunks /*[host]*/, void* stream);

/* ---------------------------------------------------------------------------------------
 * Decoder layer as channel-group kernels (csrc/decoder_layer.hip) -- replaces, for bead graphs of at most 16 nodes, the
 * per-layer launch chain of the pseudo-vector decoder loop cgvae.py:100-123: EquiMessagePsuedo (conv.py:180-242) with
 * its inv_dense.1 product (conv.py:63-75), UpdateBlock (conv.py:588-616) with the u_mat / v_mat and s_dense.1 products,
 * the residual adds (cgvae.py:108-111, 122-123) and their autograd backward.  A block owns 4 channels f0..f0+3 and the
 * weight rows {g F + f} that feed them; grid = F / 4 blocks of 576 threads.
 * Slices (outputs of the backward phases; inputs of the next one): slice s = block s's row-split partial product,
 * QUAD-MAJOR [K/4][rows][4] floats (rows = n, or 3 n behind uv_bwd), cgv_decoder_slice_floats(K, rows) each;
 * n_slices = F/4 (N/4 for dense_bwd).  The message kernels stage the bead graph in LDS: their `n_edges` argument is the
 * number of edge RECORDS TO STAGE (1..cgv_decoder_max_edges(); the record / index arrays must hold that many) -- pass the
 * arrays' capacity, not a batch's edge count: the edge structure itself is read from rowptr on the device, so the same
 * launch (a captured graph node) serves batches with other edge counts; edges beyond the staged records are ignored.
 *   forward   msg_fwd   phi = a1 W2^T + b2 -> message -> stack[:, :F] = S', Sbar', V', Vbar', V' as rows [3n, F]
 *             uv_fwd    UV [3n, 2F] = rows [Wu; Wv]^T ; stack[:, F:] = sqrt(sum_xyz (Vv^2 + 1e-10))
 *             gate_fwd  a [n, 3F] = a0 W1'^T + b1' ; S'' = S' + (U.Vv) a_sv + a_ss ; V'' = V' + U a_vv
 *   backward  gate_bwd  gS = gs_base + sum gs_slices (written to gs_sum) ; ga, gUV (gU | gVv) ; slices = ga W1'
 *             dense_bwd g = sum g_slices (written to g_dense) ; slices = (g act'(z)) W      (W [N, K], grid N/4)
 *             uv_bwd    g_stack = sum slices ; g_s2 = g_stack[:, :F] + gs_res ; gUV_out = [gUV[:, :F] | gUV[:, F:] + g_stack[:, F:] Vv / norm]
 *                       (gUV_out may be gUV itself only with CGV_OPT_DECODER_COLSPLIT = 0) ; slices [.., 48 rows ..] = gUV_out [Wu; Wv]
 *             msg_bwd   gV' = sum gvrows_slices (rows 3i+xyz) + gv_res ; full EquiMessagePsuedo backward (g_s, g_sbar,
 *                       g_v, g_vbar, g_phi, gWd, gbd written completely) ; slices = g_phi W2
 *             slices_to_dense  out [n, F] = base + sum slices (16-row slices)
 * ------------------------------------------------------------------------------------- */
int cgv_decoder_layer_supported(int n_nodes, int n_feat, int n_rbf);
int64_t cgv_decoder_slice_floats(int K, int rows);
int cgv_decoder_max_edges(void);
int cgv_decoder_block_channels(int width);   /* 4 or 8: gate_bwd / dense_bwd / uv_bwd emit width / this slices */
int cgv_decoder_debug_clock(uint64_t* buf /*device, 272 slots, or NULL*/);   /* measurement only */
int cgv_decoder_msg_fwd(const float* a1, const float* W2, const float* b2, const float* s, const float* sbar, const float* v,
                        const float* vbar, const float* geom_d, const int32_t* rowptr_d, const int32_t* src_d, const float* Wd,
                        const float* bd, float* phi, float* stack, float* sbar_out, float* v_out, float* vbar_out,
                        float* rows_out, int n_nodes, int n_feat, int n_rbf, int n_edges, void* stream);
/* An EquiMessageBlock layer (conv.py:505-563 with the residual adds of CGprior.forward, cgvae.py:391-392: h += ds, v += dv)
 * on a SMALL graph (<= 16 nodes, <= cgv_decoder_max_edges() edges: the prior's bead graph) in the channel-group scheme of the
 * decoder layer: forward = cgv_decoder_dense_fwd (a1 = swish(h W1^T + b1)) + cgv_prior_msg_fwd (phi = a1 W2^T + b2 for the
 * block's 3 x 4 rows, then the message on its channels: s_out = s + ds, v_out = v + dv; with_dv = 0 leaves v_out = v);
 * backward = cgv_prior_msg_bwd + cgv_decoder_dense_bwd.  The backward is the SCALAR path only: it is for callers that never
 * use v_out's gradient (the prior and the encoder discard the vector channel, cgvae.py:393-396), so g_q0 = g_q2 = 0 and
 * the dead filter slices get explicit zero gradients.  The upstream gradient d loss / d s_out arrives as base (dense, or
 * NULL) + quad-major slices (or NULL) like every slice consumer here; g_h = their sum (dense: the residual path), g_phi
 * [n, 3F] dense for the weight-gradient launch, slices_out: n_feat / 4 slices of cgv_decoder_slice_floats(n_feat, n). */
int cgv_prior_msg_fwd(const float* a1, const float* W2, const float* b2, const float* s, const float* v, const float* geom_d,
                      const int32_t* rowptr_d, const int32_t* src_d, const float* Wd, const float* bd, float* phi, float* s_out,
                      float* v_out, int n_nodes, int n_feat, int n_rbf, int n_edges, int with_dv, void* stream);
int cgv_prior_msg_bwd(const float* phi, const float* geom_s, const int32_t* rowptr_s, const int32_t* dst_s, const float* Wd,
                      const float* bd, const float* gh_base, const float* gh_slices, int gh_n_slices, int64_t gh_slice_floats,
                      const float* W2, float* g_phi, float* g_h, float* gWd, float* gbd, float* slices_out,
                      int64_t out_slice_floats, int n_nodes, int n_feat, int n_rbf, int n_edges, void* stream);
/* y = act(x W^T + b) (z = pre-activation or NULL) for <= 16 rows, N / 4 blocks: the two full-width products of a layer */
int cgv_decoder_dense_fwd(const float* x, const float* W /*[N,K]*/, const float* bias, float* y, float* z, int n_nodes, int N,
                          int K, int act, void* stream);
int cgv_decoder_uv_fwd(const float* rows, const float* Wuv, float* UV, float* stack, int n_nodes, int n_feat, void* stream);
int cgv_decoder_gate_fwd(const float* a0, const float* W1p, const float* b1p, const float* UV, const float* stack,
                         const float* v2, float* a, float* s3, float* v3, int n_nodes, int n_feat, void* stream);
/* (A forward of the UpdateBlock with both element-wise halves in channel-group epilogues, for 17..96 bead rows, measured
 * slower than product + element-wise launch on the dipeptide and the 2000-atom graph and was removed; commit 028bd3e last
 * held it.) */
int cgv_decoder_gate_bwd(const float* UV, const float* a, const float* gs_base /*or NULL*/, const float* gs_slices /*or NULL*/,
                         int gs_n_slices, int64_t gs_slice_stride, const float* gv /*or NULL*/, const float* W1p, float* ga,
                         float* gUV, float* gs_sum, float* slices_out, int64_t out_slice_stride, int n_nodes, int n_feat,
                         void* stream);
int cgv_decoder_dense_bwd(const float* g_slices, int g_n_slices, int64_t g_slice_stride, const float* z /*or NULL*/, int act,
                          const float* W, float* g_dense, float* slices_out, int64_t out_slice_stride, int n_nodes, int N, int K,
                          void* stream);
int cgv_decoder_uv_bwd(const float* gstack_slices, int n_slices, int64_t slice_stride, const float* UV, const float* stack,
                       const float* gs_res, const float* Wuv, const float* gUV, float* gUV_out, float* g_s2, float* slices_out,
                       int64_t out_slice_stride, int n_nodes, int n_feat, void* stream);
int cgv_decoder_msg_bwd(const float* phi, const float* s, const float* sbar, const float* v, const float* vbar,
                        const float* geom_d, const int32_t* rowptr_d, const int32_t* src_d, const float* geom_s,
                        const int32_t* rowptr_s, const int32_t* dst_s, const float* Wd, const float* bd, const float* gh,
                        const float* ghb /*or NULL*/, const float* gvrows_slices, int n_slices, int64_t slice_stride,
                        const float* gv_res /*or NULL*/, const float* gvb /*or NULL*/, const float* W2, float* g_phi, float* g_s,
                        float* g_sbar, float* g_v, float* g_vbar, float* gWd, float* gbd, float* slices_out,
                        int64_t out_slice_stride, int n_nodes, int n_feat, int n_rbf, int n_edges, void* stream);
int cgv_decoder_slices_to_dense(const float* base /*or NULL*/, const float* slices, int n_slices, int64_t slice_stride,
                                float* out, int n_nodes, int n_feat, void* stream);

/* ---------------------------------------------------------------------------------------
 * K5  UpdateBlock element-wise core (conv.py:588-616); the K=F products are separate launches
 * (skinny GEMMs below / hipBLASLt).  U, Vv = u_mat / v_mat applied to v as rows r = node*3 + xyz with row
 * stride `ld` floats (ld = F for separate buffers, 2F when both are column halves of one product with
 * the concatenated weights [u_mat; v_mat]); a = s_dense(stack) viewed [N,3,F] = (a_vv, a_sv, a_ss).
 *   rows_from_vec : rows[n,k,f] = v[n,f,k]                                          conv.py:591
 *   vec_from_rows : vec[n,f,k] = rows[n,k,f] (+ res[n,f,k])                         (its backward, + residual pass-through)
 *   norm_stack    : stack[n] = [ s[n,:] | sqrt(sum_k (Vv[n,k,:]^2 + 1e-10)) ]       conv.py:600-601
 *   gate          : dv[n,f,k] = U[n,k,f] a_vv ; ds[n,f] = (sum_k U Vv) a_sv + a_ss  conv.py:607-614
 *                   with s_res / v_res: s + ds and v + dv (cgvae.py:122-123) instead of the deltas
 * and the backward kernels (g_ds / g_dv / g_res may be NULL; norm_stack_bwd can accumulate onto gVv).
 * ------------------------------------------------------------------------------------- */
int cgv_update_rows_from_vec(const float* v /*[N,F,3]*/, float* rows /*[N,3,F]*/, int n_nodes, int n_feat, void* stream);
int cgv_update_vec_from_rows(const float* rows, const float* res /*[N,F,3] or NULL*/, float* vec, int n_nodes, int n_feat,
                             void* stream);
int cgv_update_norm_stack_fwd(const float* s /*[N,F]*/, const float* Vv, float* stack /*[N,2F]*/, int n_nodes, int n_feat,
                              int ld, void* stream);
int cgv_update_norm_stack_bwd(const float* gstack, const float* Vv, const float* stack, const float* g_res /*[N,F] or NULL*/,
                              float* g_s, float* gVv, int n_nodes, int n_feat, int ld, int accumulate, void* stream);
int cgv_update_gate_fwd(const float* U, const float* Vv, const float* a, const float* s_res /*[N,F] or NULL*/,
                        const float* v_res /*[N,F,3] or NULL*/, float* ds /*[N,F]*/, float* dv /*[N,F,3]*/,
                        int n_nodes, int n_feat, int ld, void* stream);
int cgv_update_gate_bwd(const float* U, const float* Vv, const float* a, const float* g_ds, const float* g_dv,
                        float* gU, float* gVv, float* ga, int n_nodes, int n_feat, int ld, void* stream);

/* ---------------------------------------------------------------------------------------
 * Skinny fp32 GEMMs for the node-level Dense / nn.Linear layers on the bead graph
 * (modules.py:103-114, Swish modules.py:16-21, and their autograd backward): M <=
 * cgv_skinny_max_rows() rows, weight W[N,K] row-major as torch stores it, N % 4 == 0,
 * K % 4 == 0, 16-byte aligned operands.  act: 0 = identity, 1 = Swish, 2 = tanh, 3 = ReLU (nn.Tanh / nn.ReLU of the mu / sigma heads),
 * 4 = 1e-12 + exp(z/2) (sigma head, cgvae.py:503), 5 = 1e-9 + exp(z/2) (prior std, cgvae.py:401).
 *   fwd        z = x W^T + bias ; y = act(z)      (bias may be NULL; z [M,N] is written when act != 0)
 *   bwd_input  gx[M,K] = (gy * act'(z)) W         (deterministic).  With a workspace of
 *              cgv_skinny_bwd_input_workspace_bytes bytes (contents ignored) the weight rows are
 *              split over ~320 blocks whose partial sums a second small launch adds in a fixed
 *              order; with ws = NULL one block per 64 output columns walks all rows (one launch,
 *              slow, same result up to summation order).
 *   grouped weight gradients: the caller queues one 88-byte record per layer
 *       { gy, x, z, gW, gb (pointers), M, N, K, accumulate, act, block_begin, tiles_k, tile_w, seg_rows, seg_stride, pad }
 *     (tiles_k / tile_w / the block count come from cgv_wgrad_plan; block_begin is the running sum
 *     of the block counts) and ONE cgv_grouped_wgrad launch computes, for every record,
 *       gW[N,K] (+)= (gy * act'(z))^T x ,  gb[N] (+)= sum_m (gy * act'(z))[m,:]     (gb may be NULL)
 *     max_lds_floats = max over records of cgv_wgrad_lds_floats(M, tile_w).
 * v_mfma_f32_16x16x4_f32 is an exact fp32 FMA chain, so these match an fmaf loop bit for bit.
 * ------------------------------------------------------------------------------------- */
int cgv_skinny_max_rows(void);
int cgv_skinny_supported(int M, int N, int K);
int cgv_skinny_fwd_supported(int M, int N, int K);   /* cgv_skinny_linear_fwd alone: any row count (row blocks over blockIdx.y) */
int cgv_skinny_linear_fwd(const float* x, const float* W, const float* bias, float* y, float* z /*or NULL*/, int M, int N,
                          int K, int act, void* stream);
int cgv_skinny_bwd_input_supported(int M, int N, int K);      /* bwd_input alone takes up to 128 rows */
size_t cgv_skinny_bwd_input_workspace_bytes(int M, int N, int K);
int cgv_skinny_linear_bwd_input(const float* gy, const float* z /*or NULL*/, const float* W, float* gx, int M, int N, int K,
                                int act, void* ws /*or NULL*/, size_t ws_bytes, void* stream);
/* the same with a second gradient of the input added in the reduction launch of the row-split product; returns
 * CGV_E_UNSUPPORTED when the product has one row slice only (no reduction launch): add separately then. */
int cgv_skinny_linear_bwd_input_add(const float* gy, const float* z /*or NULL*/, const float* W, const float* add, float* gx,
                                    int M, int N, int K, int act, void* workspace, size_t workspace_bytes, void* stream);
/* ... and with the result multiplied by act_out'(z_out), z_out [M, K] the pre-activation of the layer that produced this
 * layer's input (add may be NULL): see cgv_tile_linear_bwd_input_out.  CGV_E_UNSUPPORTED for a single row slice. */
int cgv_skinny_linear_bwd_input_out(const float* gy, const float* z /*or NULL*/, const float* W, const float* add /*or NULL*/,
                                    float* gx, int M, int N, int K, int act, const float* z_out, int act_out, void* workspace,
                                    size_t workspace_bytes, void* stream);
/* Dense backward prologue for any row count (the library-GEMM path of the atom-level layers):
 *   g = gy * act'(z)  (stored to g_out [M,N] when act != 0 and g_out != NULL)  and
 *   gb[n] (+)= sum_m g[m,n]  (gb may be NULL) -- one launch, fixed summation order.
 * Replaces the tensor-op chain of modules.py:16-21's autograd backward plus the bias column sum. */
int cgv_dense_grad_prepare(const float* gy, const float* z /*or NULL*/, float* g_out /*or NULL*/, float* gb /*or NULL*/,
                           int M, int N, int act, int accumulate, void* stream);
/* Tiled fp32 GEMMs for the same layers at any row count (atom-level layers, M = atoms of the batch):
 * the reduction axis of every block is split over its 4 waves, operands are loaded from L2 directly in
 * MFMA layout, bias + Swish are fused into the forward epilogue.  Need N % 4 == 0, K % 4 == 0 and
 * 16-byte aligned x / W / g / gx / gW.  g is the activation-corrected upstream gradient
 * (cgv_dense_grad_prepare).  Exact fp32 FMA chains; deterministic. */
int cgv_tile_supported(int M, int N, int K);
int cgv_tile_linear_fwd(const float* x, const float* W, const float* bias /*or NULL*/, float* y, float* z /*or NULL*/, int M,
                        int N, int K, int act, void* stream);
int cgv_tile_linear_bwd_input(const float* g, const float* W, float* gx, int M, int N, int K, void* stream);
/* the same with g = gy * act'(z) formed in the operand loads (saves the cgv_dense_grad_prepare pass when the weight /
 * bias gradients go to the grouped launch, which applies act' and sums the bias itself) */
int cgv_tile_linear_bwd_input_act(const float* gy, const float* z /*or NULL*/, const float* W, float* gx, int M, int N, int K,
                                  int act, void* stream);
/* gx = add + (gy * act'(z)) W  (add [M, K]: a second gradient of the layer's input, e.g. the residual / message-kernel path of
 * a block whose first Dense reads the same state -- conv.py:63-75 + 553-561: the accumulation autograd would do with a
 * separate add launch rides in the store epilogue). */
int cgv_tile_linear_bwd_input_act_add(const float* gy, const float* z /*or NULL*/, const float* W, const float* add, float* gx,
                                      int M, int N, int K, int act, void* stream);
/* ... and a third gradient held as ONE ROW PER SEGMENT of the rows -- the backward of scatter_mean / scatter_add of this
 * very input (cgvae.py:297): gx[m, :] += seg_grad[row2seg[m], :] (/ max(len(segment), 1) when mean) in the store epilogue,
 * instead of cgv_segment_broadcast + an accumulation add.  add may be NULL. */
int cgv_tile_linear_bwd_input_act_add_bcast(const float* gy, const float* z, const float* W, const float* add, const float* seg_grad,
                                            const int64_t* row2seg, const int32_t* seg_rowptr, int mean, float* gx, int M, int N,
                                            int K, int act, void* stream);

/* PAIR launches of the tile kernels: two Dense layers of ONE shape (M, N, K; each with its own activation code) in one grid (the extra grid dimension
 * selects the operands).  Replaces two consecutive layer launches whose inputs are ready at the same time: the first Dense
 * of ContractiveMessageBlock i and of EquiMessageBlock i + 1 read the same atom state (cgvae.py:286-305, conv.py:512-516 /
 * 709-713), their second Dense layers follow together; in backward the two second layers' input gradients.
 * cgv_tile_pair_supported: does this shape run on the register-tile kernels (the LDS-staged ones of big shapes take no pair)? */
int cgv_tile_pair_supported(int M, int N, int K);
int cgv_tile_pair_linear_fwd(const float* x_a, const float* W_a, const float* bias_a, float* y_a, float* z_a, const float* x_b,
                             const float* W_b, const float* bias_b, float* y_b, float* z_b, int M, int N, int K, int act_a,
                             int act_b, void* stream);
int cgv_tile_pair_linear_bwd_input(const float* gy_a, const float* z_a, const float* W_a, const float* add_a, float* gx_a,
                                   const float* gy_b, const float* z_b, const float* W_b, const float* add_b, float* gx_b, int M,
                                   int N, int K, int act_a, int act_b, void* stream);
/* The two entry points above whose OUTPUT is multiplied by act_out'(z_out) -- z_out [M, K] = the pre-activation of the layer
 * that produced this layer's input (modules.py:103-114: y = act(z)), so the stored gx is that layer's g = gy * act'(z)
 * and its own backward runs with act = 0.  Applied once per element in the store epilogue instead of in the operand loads
 * of the producing layer's backward-input and weight-gradient launches (every column-tile block of a row tile evaluates
 * it again there).  add may be NULL; in the pair form either z_out may be NULL (that output is stored as it is). */
/* UpdateBlock.forward's backward (conv.py:600-603) through s_dense.0 AND the norm / stack step in ONE launch: the product
 * g_stack = (gy * act'(z)) W over M beads (K = 2 F columns) is not stored; columns k < F become g_s = g_stack + g_res (g_res
 * may be NULL), columns F + f go through d ||Vv|| / d Vv: gVv[3 m + xyz, f] (+)= g_stack / stack[m, F + f] * Vv[3 m + xyz, f]
 * (rows of ld floats; accumulate != 0 adds to what cgv_update_gate_bwd left there).  Replaces cgv_tile_linear_bwd_input_act +
 * cgv_update_norm_stack_bwd. */
int cgv_tile_linear_bwd_input_norm_stack(const float* gy, const float* z, const float* W, int M, int N, int K, int act,
                                         const float* stack, const float* Vv, const float* g_res, float* g_s, float* gVv, int ld,
                                         int accumulate, void* stream);
/* What cgv_tile_linear_bwd_input* would do for this shape GIVEN a registered workspace (the workspace is per (host thread,
 * stream) state a single call cannot see): *shares = blocks per output tile of the split reduction (1 = unsplit), *streamk = 1 when
 * the stream-K kernel takes the launch (np = 1: single, 2: pair launch).  For callers that choose between these entry points and
 * the row-split kernel of cgv_skinny_linear_bwd_input. */
int cgv_tile_bwd_input_plan(int M, int N, int K, int np, int* shares /*[host]*/, int* streamk /*[host]*/);
/* Few output tiles and a long reduction (96 bead rows x 1800 columns: 60 tiles on 256 CUs): with a workspace registered the
 * backward-input launches of the CALLING host thread on `stream` give such a tile to 2 - 4 blocks, each with a share of the
 * reduction; their partial tiles meet in the workspace and the last block to arrive adds them in share order and runs the
 * store epilogue (results do not depend on timing).  ws: >= 64 KB + 2 MB, 16-byte aligned, ZERO-FILLED once by the caller
 * (self-resetting tickets at its head), used by one stream at a time; NULL unregisters. */
int cgv_tile_bwd_input_split(void* workspace, size_t workspace_bytes, void* stream);
int cgv_tile_linear_bwd_input_out(const float* gy, const float* z, const float* W, const float* add, float* gx, int M, int N,
                                  int K, int act, const float* z_out, int act_out, void* stream);
int cgv_tile_pair_linear_bwd_input_out(const float* gy_a, const float* z_a, const float* W_a, const float* add_a, float* gx_a,
                                       const float* gy_b, const float* z_b, const float* W_b, const float* add_b, float* gx_b,
                                       int M, int N, int K, int act_a, int act_b, const float* z_out_a, int act_out_a,
                                       const float* z_out_b, int act_out_b, void* stream);
/* gx = add + (gy_a * act_a'(z_a)) W_a + (gy_b * act_b'(z_b)) W_b [+ seg_grad spread over the rows]: the input gradient of two
 * layers of one shape that read the SAME input, as one product with two sources (the first Dense of ContractiveMessageBlock i
 * and of EquiMessageBlock i + 1, cgvae.py:286-305); add / seg_grad may be NULL, seg_* as in
 * cgv_tile_linear_bwd_input_act_add_bcast. */
int cgv_tile_linear_bwd_input_sum2(const float* gy_a, const float* z_a, const float* W_a, const float* gy_b, const float* z_b,
                                   const float* W_b, const float* add, const float* seg_grad, const int64_t* row2seg,
                                   const int32_t* seg_rowptr, int mean, float* gx, int M, int N, int K, int act_a, int act_b,
                                   void* stream);
int cgv_tile_linear_wgrad(const float* g, const float* x, float* gW, int M, int N, int K, int accumulate, void* stream);
int cgv_wgrad_record_bytes(void);
int cgv_wgrad_plan(int M, int N, int K, int* tiles_k /*[host]*/, int* tile_w /*[host]*/, int* n_blocks /*[host]*/);
int cgv_wgrad_lds_floats(int M, int tile_w);
int cgv_grouped_wgrad(const void* table_dev, int n_problems, int total_blocks, int max_lds_floats, void* stream);
/* Data-parallel OPERAND exchange for the same layers.  A weight gradient g^T x has rank <= rows; the bead-level
 * layers have 12 rows per GPU against 0.36 - 3.2 M weights, so instead of all-reducing gW (270 MB per step on the
 * chignolin config) the ranks all-gather their operand rows and each forms the global gradient -- exactly what one
 * process computes on the concatenated batch (the reference's single-process step, scripts/utils.py:110-157).
 *   cgv_pack_operands: one launch copies, for every 64-byte record
 *       { gy, z, x, dst_g, dst_x (pointers), M, N, K, act, block_begin, pad }
 *     dst_g[M,N] = gy * act'(z), dst_x[M,K] = x into the caller's send buffer (block counts: cgv_pack_plan).
 *   cgv_grouped_wgrad_gathered: the 88-byte record of cgv_grouped_wgrad with act = 0, z = NULL and
 *     seg_rows (rows per rank, a multiple of 4) / seg_stride (floats between the rank segments of the gathered
 *     buffer): row m of the problem is row m % seg_rows of segment m / seg_rows; M = ranks * seg_rows (any size).
 *     tiles_k / the block count come from cgv_wgrad_gathered_plan; tile_w is unused.  Output tiles of 64 rows x 128 columns, exact
 *     fp32 MFMA chains in a fixed order: every rank obtains bit-identical gradients. */
int cgv_wgrad_gathered_plan(int M, int N, int K, int seg_rows, int* tiles_k /*[host]*/, int* n_blocks /*[host]*/);
int cgv_grouped_wgrad_gathered(const void* table_dev, int n_problems, int total_blocks, void* stream);
/* tile = 64 | 128: edge of the output tiles (records planned with the same tile); 128 x 128 halves the operand traffic
 * per gW element but measured slower on the shapes of this model -- an opt-in variant */
int cgv_wgrad_gathered_plan_tile(int M, int N, int K, int seg_rows, int tile, int* tiles_k /*[host]*/, int* n_blocks /*[host]*/);
int cgv_grouped_wgrad_gathered_tile(const void* table_dev, int n_problems, int total_blocks, int tile, void* stream);
/* The same grouped weight gradients (table and plan of tile = 128) on the bf16 matrix path with SPLIT operands: every fp32
 * operand value as the exact sum of three bf16 terms, six bf16 MFMA products per fp32 product, fp32 accumulation --
 * fp32-class accuracy (dropped terms < 2^-23 of a product) at 3/8 of the fp32 MFMA time.  Replaces the autograd weight
 * gradients of nn.Linear / Dense (modules.py Dense, conv.py:505-563 inv_dense) on layers with more than 128 operand rows. */
int cgv_grouped_wgrad_split(const void* table_dev, int n_problems, int total_blocks, void* stream);
/* Rank update over gathered operand rows with MFMA tiles -- for layers whose gathered row count is beyond the range in
 * which the FMA-per-row kernel (cgv_grouped_wgrad_adam) pays (~40 rows: 4+ data-parallel ranks of 12 bead rows, or the
 * 36-row [u_mat; v_mat] layers at 2+).  Same records and plan as cgv_grouped_wgrad_gathered (tile 64; accumulate = 0).
 * _sumsq: the tiles are formed and squared, never stored: sumsq[i] = ||gW_i||_F^2 (block partials in `partial`:
 * total_blocks doubles, summed per record in block order); the bias gradients are written.  _adam: the tiles are
 * formed again and go, clipped, through the Adam update of their weights (state from cgv_optim_prepare_extra over
 * those norms); every gW must lie inside the gradient arena, p / m / v are addressed through its offset there.
 * Replaces, for those layers and data-parallel training, Dense's weight gradient (modules.py:103-114) +
 * clip_grad_norm_ + Adam.step (scripts/utils.py:150-157) on the all-gathered batch. */
int cgv_grouped_wgrad_gathered_sumsq(const void* table_dev, int n_problems, int total_blocks, double* partial, double* sumsq,
                                     void* stream);
int cgv_grouped_wgrad_gathered_adam(const void* table_dev, int n_problems, int total_blocks, const float* arena_g,
                                    float* arena_p, float* arena_m, float* arena_v, float lr, float beta1, float beta2,
                                    float eps, const float* state, void* stream);
/* Strip layout of the three gathered launches, for records of at most cgv_wgrad_strip_max_rows() (128) operand rows:
 * one block per 64 ROWS of gW, which stages its g columns once and walks the strip's K / 64 column tiles with the next
 * x tile loading under the current tile's MFMAs (the tile layout above gives each 64 x 64 tile a block of its own that
 * spends most of its life on its first loads).  Records as above with block_begin counted in strip blocks
 * (cgv_wgrad_strip_plan: ceil(N / 64)); tiles_k / tile_w unused.  max_rows = the largest M of the table (sizes the LDS).
 * Bit-identical to the tile layout: same MFMA chains in the same row order. */
int cgv_wgrad_strip_max_rows(void);
int cgv_wgrad_strip_plan(int M, int N, int K, int seg_rows, int* n_blocks /*[host]*/);
int cgv_grouped_wgrad_strip(const void* table_dev, int n_problems, int total_blocks, int max_rows, void* stream);
/* The strip layout on the bf16 matrix path with split operands (fp32-class accuracy, see cgv_grouped_wgrad_split): for
 * records of at most cgv_wgrad_strip_split_max_rows() (96) rows.  x is split ONCE per problem into three bf16 planes in `ws`
 * (record field `pad` = the problem's offset in ws in 256-byte units; cgv_wgrad_strip_split_plane_bytes(M, K) bytes each),
 * g = gy * act'(z) once per strip in registers; the strips then walk their column tiles without arithmetic on the operands.
 * max_rows / max_k: the largest M / K of the table.  modules.py:103-114 (autograd of Dense: gW = g^T x, gb = sum_m g). */
int cgv_wgrad_strip_split_max_rows(void);
size_t cgv_wgrad_strip_split_plane_bytes(int M, int K);
int cgv_grouped_wgrad_strip_split(const void* table_dev, int n_problems, int total_blocks, int max_rows, int max_k, void* ws,
                                  size_t ws_bytes, void* stream);
int cgv_grouped_wgrad_strip_sumsq(const void* table_dev, int n_problems, int total_blocks, int max_rows, double* partial,
                                  double* sumsq, void* stream);
int cgv_grouped_wgrad_strip_adam(const void* table_dev, int n_problems, int total_blocks, int max_rows, const float* arena_g,
                                 float* arena_p, float* arena_m, float* arena_v, float lr, float beta1, float beta2,
                                 float eps, const float* state, void* stream);
int cgv_pack_record_bytes(void);
int cgv_pack_plan(int M, int N, int K, int* n_blocks /*[host]*/);
int cgv_pack_operands(const void* table_dev, int n_problems, int total_blocks, void* stream);

/* ---------------------------------------------------------------------------------------
 * Decoder tail (cgvae.py:462-481):  xyz[a] = v[mapping[a], chan[a], :] - [offset] mean over the bead of the
 * same + cg_xyz[mapping[a]].  rowptr [n_beads+1] / atom [n_atoms]: bead -> atoms CSR (the dst-sorted view of
 * the contraction plan: cgv_csr_build on mapping, rowptr_d / eid_d); chan int64 [n_atoms] = rank of the atom
 * inside its bead (CG2ChannelIdx, cgvae.py:451-460), chan < n_feat.  bwd writes ALL of g_v [n_beads,F,3]
 * (zeros outside the addressed slots) and, when not NULL, g_cg_xyz [n_beads,3].
 * ------------------------------------------------------------------------------------- */
int cgv_reconstruct_fwd(const float* v, const float* cg_xyz, const int32_t* rowptr, const int32_t* atom, const int64_t* chan,
                        int n_beads, int n_feat, int offset, float* xyz /*[n_atoms,3]*/, void* stream);
int cgv_reconstruct_bwd(const float* g_xyz, const int32_t* rowptr, const int32_t* atom, const int64_t* chan, int n_beads,
                        int n_feat, int offset, float* g_v, float* g_cg_xyz /*or NULL*/, void* stream);

/* ---------------------------------------------------------------------------------------
 * Fused ELBO loss -- replaces KL (scripts/utils.py:81-86, incl. its (mu1-mu2)^2 / std2 term) and the
 * loss assembly of scripts/utils.py:117-141:  loss = recon + beta*KL + gamma*graph with
 *   recon = mean((xr - x)^2),  graph = mean_b((|xr_a - xr_b|_eps - |x_a - x_b|_eps)^2), eps = 1e-6 inside the sqrt.
 * out4 = { loss, KL, recon, graph }.  The same launch stores d loss / d{mu, sigma, prior_mu, prior_std,
 * xyz_recon}; cgv_elbo_scale multiplies them by the upstream scalar (device pointer) in backward.
 * bonds: int64 [n_bonds, 2] batch-global atom ids (bond_edge_list of CG_collate).
 * ------------------------------------------------------------------------------------- */
/* workspace of cgv_elbo_workspace_bytes bytes (0 for small bead batches): lets the KL terms of a large batch run on
 * their own multi-block launch; with NULL everything runs in the one-block kernel (same result up to summation order). */
size_t cgv_elbo_workspace_bytes(int n_beads, int n_feat);
int cgv_elbo_fwd(const float* mu, const float* sigma, const float* prior_mu, const float* prior_std, const float* xyz,
                 const float* xyz_recon, const int64_t* bonds, int n_beads, int n_feat, int n_atoms, int n_bonds,
                 float beta, float gamma, float* out4, float* loss_out /*[1] or NULL: the loss once more, as a tensor of
                 its own (an autograd output that is not a view of the non-differentiable terms: saves the clone)*/,
                 float* g_mu, float* g_sigma, float* g_prior_mu, float* g_prior_std, float* g_xyz_recon,
                 void* workspace /*or NULL*/, size_t workspace_bytes, void* stream);
int cgv_elbo_scale(const float* g_loss, float* g_mu, float* g_sigma, float* g_prior_mu, float* g_prior_std, int n_bead_elems,
                   float* g_xyz_recon, int n_atom_elems, void* stream);
/* Decoder tail (cgv_reconstruct_fwd: cgvae.py:462-481) + the ELBO above + BOTH their gradients in ONE launch, one block
 * per bead: xyz_recon is an OUTPUT here, and besides d loss / d{mu, sigma, prior_mu, prior_std, xyz_recon} the launch
 * leaves g_V [n_beads, F, 3] = d loss / d V (what cgv_reconstruct_bwd would compute from g_xyz_recon).  rowptr / atom_of /
 * bead_of: the atom -> bead plan (CSR by bead, atom ids and bead ids in bead-sorted order).  Sums in double, block
 * partials added in block order by the block that arrives last (device-scope ticket): deterministic.
 * workspace: cgv_loss_tail_workspace_bytes(n_beads) bytes, 16-byte aligned, ZERO before the first launch (every launch
 * leaves its ticket word at zero again).  Limits: cgv_loss_tail_supported (atoms + beads <= 3072: both coordinate sets live in LDS). */
int cgv_loss_tail_supported(int n_beads, int n_feat, int n_atoms, int n_bonds);
size_t cgv_loss_tail_workspace_bytes(int n_beads);
int cgv_loss_tail(const float* V, const float* cg_xyz, const int32_t* rowptr, const int32_t* atom_of, const int32_t* bead_of,
                  const int64_t* chan, const float* mu, const float* sigma, const float* prior_mu, const float* prior_std,
                  const float* xyz, const int64_t* bonds, int n_beads, int n_feat, int n_atoms, int n_bonds, int offset,
                  float beta, float gamma, float* xyz_recon, float* out4, float* loss_out, float* g_mu, float* g_sigma,
                  float* g_prior_mu, float* g_prior_std, float* g_xyz_recon, float* g_V, void* workspace, size_t workspace_bytes,
                  void* stream);

/* ---------------------------------------------------------------------------------------
 * Fused optimiser step over a flat fp32 arena of the parameters that receive gradients --
 * replaces the skip rule, clip_grad_norm_(params, 0.01) and Adam.step() of
 * scripts/utils.py:145-157 (torch.optim.Adam defaults: no amsgrad, no weight decay).
 *   skip   = loss >= skip_threshold || isnan(loss)         (loss == NULL: never skip)
 *   norm   = |grad_scale| * ||g||_2 ;  coef = min(1, max_norm / (norm + 1e-6))
 *   g' = g * coef * grad_scale ; m,v,p updated as Adam does ; step counter += 1
 * `state` is cgv_optim_state_floats() device floats, zero-initialised by the caller once:
 *   [0] step  [1] last grad norm  [2] clip*scale  [3] 1-b1^t  [4] sqrt(1-b2^t)  [5] skipped?  [6] #skipped
 * `partial` is cgv_optim_partial_floats() device floats of scratch, ZEROED once by the caller (its last 16 floats hold the
 * ticket word of the one-launch norm + decision pass; every launch leaves it zero).  No host synchronisation.
 * ------------------------------------------------------------------------------------- */
int cgv_optim_state_floats(void);
int cgv_optim_partial_floats(void);
int cgv_adam_clip_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                       float eps, float max_norm, float grad_scale, const float* loss /*[1] or NULL*/,
                       float skip_threshold, float* state, float* partial, void* stream);
/* Its two halves: cgv_optim_prepare = global norm, skip decision, clip coefficient, bias corrections -> `state`;
 * cgv_adam_apply = the parameter / moment pass over ONE contiguous range (pointers already offset, 16-byte aligned),
 * reading `state`.  prepare + apply over the whole arena == cgv_adam_clip_step; apply may be issued per range, on
 * another stream, and after further kernels (the trainer overlaps the decoder range's update with the next forward). */
int cgv_optim_prepare(const float* g, int64_t n, float beta1, float beta2, float max_norm, float grad_scale,
                      const float* loss /*[1] device or NULL*/, float skip_threshold, float* state, float* partial,
                      void* stream);
int cgv_adam_apply(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                   const float* state, void* stream);
/* torch.optim.SGD defaults (scripts/run_ala.py:43, `-optimizer sgd`): p -= lr * clip * g over one range, clip coefficient and
 * skip decision taken from the state cgv_optim_prepare wrote (scripts/utils.py:145-157). */
int cgv_sgd_apply(float* p, const float* g, int64_t n, float lr, const float* state, void* stream);

/* Rank-update layers (bead-level Dense / nn.Linear weights: M <= 64 operand rows against 0.36 - 3.2 M weights).  Their
 * weight gradient gW = g^T x is never written: cgv_wgrad_gram gives its squared Frobenius norm from the operands
 * (sum over row pairs of (g_a . g_b)(x_a . x_b), in double; sumsq[i] for table record i) and writes the bias gradients;
 * cgv_optim_prepare_extra is cgv_optim_prepare over the materialised part of the arena plus those norms; and
 * cgv_grouped_wgrad_adam re-forms each gW tile (the table and tiling of cgv_grouped_wgrad) and applies the clipped Adam
 * update to the weights, moments addressed through gW's offset in the gradient arena.  Replaces, for these layers,
 * Dense's autograd weight gradient (CoarseGrainingVAE/modules.py:103-114) + clip_grad_norm_ + Adam.step
 * (scripts/utils.py:150-157) with 24 instead of 36 bytes of HBM traffic per weight.  Records must have accumulate = 0.
 * The records may address GATHERED operands (seg_rows / seg_stride as for cgv_grouped_wgrad_gathered: the rows of all
 * data-parallel ranks, M = world x rows per rank): the update every rank then applies is the whole batch's, and no
 * rank ever materialises these gradients either.  max_rows: the largest M in the table (sizes the kernel's LDS). */
int cgv_wgrad_gram(const void* table_dev, int n_problems, int max_rows, double* sumsq, void* workspace,
                   size_t workspace_bytes, void* stream);
size_t cgv_wgrad_gram_workspace_bytes(int n_problems);
/* cgv_wgrad_gram for records of up to cgv_wgrad_gram_mfma_max_rows() = 128 rows (gathered rows of 4 - 8 ranks, bead rows
 * of a large batch): the Gram matrices come from fp64 MFMA tiles instead of a walk over row pairs (same doubles). */
int cgv_wgrad_gram_mfma(const void* table_dev, int n_problems, int max_rows, double* sumsq, void* workspace,
                        size_t workspace_bytes, void* stream);
size_t cgv_wgrad_gram_mfma_workspace_bytes(int n_problems, int max_rows);
int cgv_wgrad_gram_mfma_max_rows(void);
int cgv_rank_update_supported(int M, int N, int K);   /* 1 when a layer with M operand rows can take this path (M <= 64) */
int cgv_optim_prepare_extra(const float* g, int64_t n, const double* extra, int n_extra, float beta1, float beta2,
                            float max_norm, float grad_scale, const float* loss, float skip_threshold, float* state,
                            float* partial, void* stream);
int cgv_grouped_wgrad_adam(const void* table_dev, int n_problems, int total_blocks, int max_lds_floats,
                           const float* arena_g, float* arena_p, float* arena_m, float* arena_v, float lr, float beta1,
                           float beta2, float eps, const float* state, void* stream);
/* cgv_grouped_wgrad_adam with the FLAT block layout, for records of at most 16 operand rows: the update is elementwise over
 * a weight's contiguous [N, K] array, so a block takes a contiguous range of q4 float4 of it (whole 128-byte lines of
 * p / m / v, each read and written exactly once) with x for all K columns and the g rows of its range in LDS, instead of
 * 64 rows x one k tile (row segments at a stride of K floats, whose border lines neighbouring blocks fetch twice).  Same
 * sum order over the operand rows: results are bit-identical to cgv_grouped_wgrad_adam.
 *   cgv_rank_flat_quantum   default q4 (float4 per block; any multiple of 2048 is accepted, 0 = this default)
 *   cgv_rank_flat_plan      blocks / LDS floats of one record; CGV_E_UNSUPPORTED when the shape does not take the layout
 *                           (more than 16 rows, or x [M, K] + g beyond the LDS budget) -- the launch then stays with
 *                           cgv_grouped_wgrad_adam.  A table's block_begin is the prefix of THESE block counts.
 * Replaces, like cgv_grouped_wgrad_adam, the autograd weight gradient of the bead-level nn.Linear / Dense layers
 * (modules.py Dense) + torch.optim.Adam.step on them (scripts/run_ala.py:147, utils.py:157). */
int cgv_rank_flat_quantum(void);
int cgv_rank_flat_plan(int M, int N, int K, int q4, int* n_blocks /*[host]*/, int* lds_floats /*[host]*/);
int cgv_grouped_wgrad_adam_flat(const void* table_dev, int n_problems, int total_blocks, int max_lds_floats, int q4,
                                const float* arena_g, float* arena_p, float* arena_m, float* arena_v, float lr, float beta1,
                                float beta2, float eps, const float* state, void* stream);
/* Both layouts in ONE launch: records [0, n_flat) flat (flat_blocks blocks, block prefix from 0), records [n_flat, n_problems)
 * tiled as for cgv_grouped_wgrad_adam (tiled_blocks blocks, their own prefix from 0).  The tiled records are layers of
 * more operand rows (36: three stacked heads), bound by the FMAs that form a tile rather than by p / m / v: their blocks are
 * dealt evenly among the flat ones, so they run beside blocks that wait for memory.  max_lds_floats: the larger request. */
int cgv_grouped_wgrad_adam_mixed(const void* table_dev, int n_flat, int n_problems, int flat_blocks, int tiled_blocks,
                                 int max_lds_floats, int q4, const float* arena_g, float* arena_p, float* arena_m,
                                 float* arena_v, float lr, float beta1, float beta2, float eps, const float* state,
                                 void* stream);

/* ---------------------------------------------------------------------------------------
 * K12  sample quality -- replaces, for a whole evaluation chunk in one launch, get_bond_graphs / compare_graph /
 * count_valid_graphs / compute_rmsd (scripts/sampling.py:120-239, called per sample by eval_sample_qualities,
 * sampling.py:324-333, from sample_single and get_all_true_reconstructed_structures, scripts/utils.py:193-268), which
 * build four dense [n,n] distance matrices per sample on the host.  Here no [n,n] tensor exists.
 *   ref_xyz  [n_atoms,3]               the B = n_frames reference frames, frame f = rows frame_ptr[f] .. frame_ptr[f+1]
 *   gen_xyz  [n_samples * n_atoms,3]   FRAME-major, sample-major inside a frame: sample k of frame f (n_f atoms) is rows
 *                                      n_samples * frame_ptr[f] + k * n_f .. + n_f  (the order of the reference's
 *                                      sample_xyzs, sampling.py:380, and of a disjoint-union decoder batch built that way)
 *   cls      [n_atoms] int32           element class of each atom: index into thr_sq (clamped to [0, n_classes))
 *   heavy    [n_atoms] int32           != 0: the atom belongs to the heavy-atom graph (z != 1, sampling.py:135-146)
 *   thr_sq   [n_classes,n_classes]     SYMMETRIC; atoms i != j of classes a, b are bonded iff
 *                                        s = (dx*dx + dy*dy) + dz*dz  <=  thr_sq[a][b]     (fp32, no FMA contraction)
 *                                      with thr_sq = the largest fp32 whose host sqrt is < (r_a + r_b) * scale, computed by
 *                                      the caller (graph.cutoff_threshold_sq(strict=True)): membership is bit-identical to
 *                                      the reference's `sqrt(s) < cutoff` without depending on the device sqrt (as K0).
 *   max_frame_atoms                    the largest n_f (sizes the grid; known to the caller, who built frame_ptr)
 * Outputs per (frame f, sample k), row f * n_samples + k (both buffers are zeroed by the call):
 *   counts [.,6] int32   diff_all, diff_heavy      entries where the sample's bond matrix differs from the reference's
 *                        signed_all, signed_heavy  sum(ref - gen)  (the reference takes abs of the SIGNED sum, sampling.py:189)
 *                        refsum_all, refsum_heavy  sum(ref)
 *                        -- exact, independent of the order of the launch's blocks (integer vector atomics)
 *   sums   [.,2] fp64    sum |gen - ref|^2 over all atoms / over heavy atoms, accumulated in double from
 *                        double(gen) - double(ref) in a fixed order (bitwise reproducible)
 * One launch for the chunk: a wave per (frame, sample, pair of 64-atom tiles), from 22-atom frames (one wave each) to
 * 2000-atom frames (528 waves per sample).  n_classes <= cgv_sample_quality_max_classes(), n_f <= 32768,
 * n_frames, n_samples <= 65535. */
int cgv_sample_quality_max_classes(void);
int cgv_sample_quality(const float* ref_xyz, const float* gen_xyz, const int32_t* frame_ptr /*[n_frames+1]*/,
                       const int32_t* cls, const int32_t* heavy, const float* thr_sq, int n_frames, int n_atoms,
                       int n_samples, int n_classes, int max_frame_atoms, int32_t* counts /*[n_frames*n_samples,6]*/,
                       double* sums /*[n_frames*n_samples,2]*/, void* stream);

/* ---------------------------------------------------------------------------------------
 * K13  coarse-graining map learner -- replaces the training loop of learn_map (CoarseGrainingVAE/datasets.py:204-249) on
 * the auto-encoder of CoarseGrainingVAE/cgae.py:8-33, `steps` optimiser steps per call:
 *   M = softmax(W + g), g = -log(E), E ~ Exp(1) (F.gumbel_softmax at temperature 1: the `tau` learn_map decrements never
 *   reaches it, cgae.py:27 -- kept); M_norm = M / colsum(M); cg = M_norm^T X; recon = D^T cg; lift = M cg;
 *   loss = mean((X - recon)^2) + reg_weight * mean_{b,i} sum_xyz (X - lift)^2   (datasets.py:229-231);
 *   backward through all of it; torch.optim.Adam (bias correction, no weight decay) on W and D.
 *   W, mW, vW [n,K]   assign_map and its Adam moments (updated in place)       D, mD, vD [K,n]   decode, likewise
 *   frames [n_frames,n,3]   every frame minus its own mean over atoms (centred by the caller, once)
 *   order  [order_len] int32   frame indices, whole epochs of n_train entries (a permutation of the training subset per
 *                           epoch, drawn by the caller).  Step s of the schedule (Adam's step count s + 1) takes entries
 *                           e * n_train + i * batch .. + min(batch, n_train - i * batch) with e = s / spe, i = s % spe,
 *                           spe = ceil(n_train / batch): the last, partial batch of an epoch is kept and the means
 *                           divide by its actual size.  The call runs steps step0 .. step0 + steps - 1.
 *   noise  optional [steps,n,K]   explicit g of this call's steps (parity tests).  NULL: generated in the kernel, stateless,
 *                           Philox4x32-10 with key = seed and counter = (atom, bead quad, step): word k % 4 of quad k / 4;
 *                           top 23 bits b -> u = (b + 0.5) / 2^23 in the open interval; g = -log(-log(u)) in fp64, rounded once.
 *                           cgv_cgae_noise writes exactly those numbers for steps step0 .. step0 + steps - 1 to out [steps,n,K].
 *   loss_log [steps,2]      (loss_recon, loss_reg) of every step of this call
 *   probe  optional         of the call's LAST step: M [n,K], dW [n,K], dD [K,n], cg_xyz [batch,K,3] (floats, in this order)
 * form: CGV_CGAE_RESIDENT -- one workgroup keeps W, D and the moments in LDS for the whole call (one launch; needs
 *   cgv_cgae_resident_fits(n, K, batch)); CGV_CGAE_STREAMED -- state in global memory, six launches per step.  Same form,
 *   inputs and seed: bit-identical results, and a call of `steps` steps equals `steps` calls of one.
 * workspace: cgv_cgae_workspace_bytes(n, K, batch, form), 256-byte aligned, contents need not survive between calls. */
#define CGV_CGAE_RESIDENT 1
#define CGV_CGAE_STREAMED 2
int cgv_cgae_resident_fits(int n, int K, int batch);
size_t cgv_cgae_workspace_bytes(int n, int K, int batch, int form);
int cgv_cgae_steps(int form, float* W, float* D, float* mW, float* vW, float* mD, float* vD, const float* frames,
                   int n_frames, const int32_t* order, int64_t order_len, int n_train, int batch, int n, int K,
                   int64_t step0, int steps, float reg_weight, double lr, double beta1, double beta2, double eps,
                   uint64_t seed, const float* noise, float* loss_log, float* probe, void* workspace,
                   size_t workspace_bytes, void* stream);
int cgv_cgae_noise(uint64_t seed, int64_t step0, int steps, int n, int K, float* out, void* stream);

/* ---------------------------------------------------------------------------------------
 * K14  ensemble check -- reference-free quality of generated ensembles: what is left to ask when only bead coordinates
 * exist (backmapping a coarse-grained trajectory) and K12 has no frame to compare with.  The reference marks the place
 * with `# compute sample diversity` (scripts/sampling.py:296) and computes nothing there.
 *   gen_xyz, frame_ptr, cls, heavy, thr_sq, max_frame_atoms    exactly as K12 (same layout, same bond test
 *                                      s = (dx*dx + dy*dy) + dz*dz <= thr_sq[a][b], fp32, no FMA contraction)
 *   bond_ptr [n_frames+1] int32        prefix sum of bonds per frame, ending at n_bonds (all zero: no bonds)
 *   bonds    [n_bonds,2]  int32        the topology: atom ids LOCAL to their frame, i < j, every pair once, ids < n_f.
 *                                      The CALLER guarantees this (the counting identity below needs unique pairs);
 *                                      an entry outside it counts as a missing bond.
 *                                      bond_ptr == NULL: no topology -- counts stay zero, only pair_sums are computed;
 *                                      cls, thr_sq and bonds may then be NULL, and heavy too (heavy sums stay zero).
 * Outputs (both buffers are zeroed by the call):
 *   counts    [n_frames,n_samples,4] int32   missing_all, extra_all, missing_heavy, extra_heavy: unordered atom pairs that
 *                        are a topology bond but not within the cutoff / within the cutoff but no topology bond; the heavy
 *                        columns restrict to pairs of two heavy atoms.  Computed as missing = Eb - H, extra = P - H from
 *                        P = pairs i < j within the cutoff (all-pairs pass, tiled as K12) and H = topology bonds within
 *                        the cutoff (a pass over the bond list); integer vector atomics, exact in any order.
 *                        A sample is valid iff missing + extra == 0.
 *   pair_sums [n_frames,n_samples,n_samples,2] fp64   [f,k,l,0] = sum over the frame's atoms of |x_k - x_l|^2,
 *                        [f,k,l,1] the same over heavy atoms; double(x_k) - double(x_l), added in atom order by one lane:
 *                        bitwise reproducible, exactly symmetric, zero diagonal, both halves written.
 * One launch for the chunk.  n_samples <= cgv_ensemble_check_max_samples() (1024), n_classes <=
 * cgv_ensemble_check_max_classes() (= K12's), n_f <= 32768, n_frames <= 65535; beyond a limit the call fails
 * (CGV_E_BADARG, cgv_last_error_string) -- nothing is clamped. */
int cgv_ensemble_check_max_classes(void);
int cgv_ensemble_check_max_samples(void);
int cgv_ensemble_check(const float* gen_xyz, const int32_t* frame_ptr /*[n_frames+1]*/, const int32_t* cls,
                       const int32_t* heavy, const float* thr_sq, const int32_t* bond_ptr /*[n_frames+1]*/,
                       const int32_t* bonds /*[n_bonds,2]*/, int n_frames, int n_atoms, int n_samples, int n_classes,
                       int max_frame_atoms, int n_bonds, int32_t* counts /*[n_frames*n_samples,4]*/,
                       double* pair_sums /*[n_frames*n_samples*n_samples,2]*/, void* stream);

/* ---------------------------------------------------------------------------------------
 * K15  internal-coordinate histograms -- the numbers behind the reference's offline distribution plots
 * (CoarseGrainingVAE/plots.py: ramachandran_plot, get_bonds, through mdtraj / pyemma): does an ensemble reproduce the
 * distribution of the data?  Per feature a histogram over all structures, per pair of torsions a joint histogram (the
 * Ramachandran map); no [n_structures, features] tensor exists.
 *   xyz    [n_structures,n_atoms,3]   structures of ONE molecule (fp32; widened on use, all arithmetic below is fp64)
 *   feat   [n_features,4] int32       atom ids p0..p3 of each feature (the first `kind` of them are read)
 *   kind   [n_features]   int32       2  bond length  |p0 - p1|
 *                                     3  angle at p1  atan2(|u x v|, u . v),  u = p0 - p1, v = p2 - p1
 *                                     4  proper torsion, mdtraj's sign:  atan2(|b2| * b1 . (b2 x b3), (b1 x b2) . (b2 x b3)),
 *                                        b1 = p1 - p0, b2 = p2 - p1, b3 = p3 - p2
 *   pairs  [n_pairs,2]    int32       (f, g): two torsion features whose joint histogram is wanted; may be NULL when
 *                                     n_pairs == 0.  A pair that names anything but two torsions counts nothing.
 * Outputs -- ZEROED BY THE CALLER, the launch ADDS (so launches over chunks of structures accumulate):
 *   counts      [n_features, n_bins + 3] int32   slots: under, n_bins bins, over, invalid
 *   pair_counts [n_pairs, n_bins2, n_bins2] int32   [p, bin of f, bin of g]
 * Binning: bin = floor((x - lo) * n_bins / (hi - lo)).
 *   bonds     [bond_lo, bond_hi): x < lo counts in under, x >= hi in over
 *   angles    [0, pi]: x == pi counts in the last bin; no under / over
 *   torsions  [-pi, pi) periodic: x == pi counts in bin 0; no under / over
 *   invalid   the feature touches a non-finite coordinate (or names an atom outside [0, n_atoms), or has an unknown
 *             kind): counted in `invalid` and in no pair
 * Exact integers, independent of the order of the launch's blocks and the same bits on every run (LDS integer atomics
 * per block, integer vector atomics of the non-zero slots into the outputs).  One launch: a block owns a tile of
 * cgv_internal_hist_feature_tile(n_bins) features or cgv_internal_hist_pair_tile(n_bins2) pairs and a range of
 * structures, whose coordinates it stages in LDS; structures of more than cgv_internal_hist_max_staged_atoms() atoms are
 * gathered from global memory by a second instance of the kernel (same results).
 * Limits: n_features <= cgv_internal_hist_max_features(), n_pairs <= .._max_pairs(), 1 <= n_bins <= .._max_bins(),
 * 1 <= n_bins2 <= .._max_bins2() (when n_pairs > 0), n_atoms <= .._max_atoms(); beyond a limit the call fails
 * (CGV_E_BADARG, cgv_last_error_string) before anything is written -- nothing is clamped or truncated. */
int cgv_internal_hist_max_features(void);
int cgv_internal_hist_max_pairs(void);
int cgv_internal_hist_max_bins(void);
int cgv_internal_hist_max_bins2(void);
int cgv_internal_hist_max_atoms(void);
int cgv_internal_hist_max_staged_atoms(void);
int cgv_internal_hist_feature_tile(int n_bins);   /* 0 outside the limits */
int cgv_internal_hist_pair_tile(int n_bins2);     /* 0 outside the limits */
int cgv_internal_hist(const float* xyz, const int32_t* feat /*[n_features,4]*/, const int32_t* kind /*[n_features]*/,
                      const int32_t* pairs /*[n_pairs,2]*/, int n_structures, int n_atoms, int n_features, int n_pairs,
                      int n_bins, int n_bins2, double bond_lo, double bond_hi, int32_t* counts /*[n_features,n_bins+3]*/,
                      int32_t* pair_counts /*[n_pairs,n_bins2,n_bins2]*/, void* stream);

/* ---------------------------------------------------------------------------------------
 * K16  time-lagged independent component analysis (TICA) -- does an ensemble populate the slow, collective states of the
 * simulation?  Replaces what the reference does offline through pyemma (CoarseGrainingVAE/postanalysis.py:25-68:
 * pairwise backbone distances, tica(lag=100) on the simulation, tica.transform of the generated structures).
 *   pairs  [d,2] int32    atom pairs (I, J); feature f of a frame is the distance of its pair, computed in fp32 as
 *                         sqrt((dx*dx + dy*dy) + dz*dz), every operation rounded on its own (no FMA contraction), the
 *                         square root correctly rounded, then widened to fp64.  An index outside [0, n_atoms) reads
 *                         atom 0 (the host wrapper refuses such tables); nothing is read out of bounds.
 * No [frames, d] feature tensor exists in memory.
 *
 * cgv_tica_moments: xyz [n_frames,n_atoms,3] is ONE contiguous, time-ordered segment.  With x_t = f(t), y_t = f(t + lag)
 * over t in [0, n_frames - lag) the call ADDS to the caller's fp64 buffers (zeroed by the caller before the first call)
 *   sum_x [d] += sum x_t   sum_y [d] += sum y_t   cxx [d,d] += sum x_t x_t^T   cyy [d,d] += sum y_t y_t^T
 *   cxy [d,d] += sum x_t y_t^T
 * n_frames <= lag adds nothing and returns 0.  Non-finite coordinates propagate into the sums.
 * Two launches: grid (tile pairs bi <= bj of 32 features, cgv_tica_moments_splits() frame ranges) x 256 threads, a
 * block stages 16 frame pairs of its tiles' features in LDS as fp64 and accumulates X_i X_j^T, Y_i Y_j^T, X_i Y_j^T and
 * X_j Y_i^T in registers with v_mfma_f64_16x16x4_f64, then writes its tiles to its range's slice of the workspace;
 * the second launch sums the ranges in ascending order into the totals and fills cxx / cyy below the diagonal from above
 * it.  No floating-point atomics: the same bits on every run, cxx and cyy exactly symmetric.
 * workspace: cgv_tica_moments_workspace_bytes(n_frames, d, lag) bytes, 8-byte aligned, contents need not survive.
 * Limits: 1 <= lag, d <= cgv_tica_max_features(), n_atoms <= cgv_tica_max_atoms(); beyond a limit the call fails
 * (CGV_E_BADARG) before any launch.  Bound: see DESIGN.md (K16 row).
 *
 * cgv_tica_project: structures xyz [n_structures,n_atoms,3] onto a fitted model, mean [d], W [d,k] fp64,
 * 1 <= k <= cgv_tica_max_components() (8).  One launch, one wave per structure.
 *   ics [n_structures,k] fp64 (may be NULL)   ics[s,c] = sum_f (f_s[f] - mean[f]) * W[f,c]: each lane sums features
 *                         lane, lane + 64, .. in ascending order, a fixed tree combines the lanes (same bits every run)
 *   counts [n_bins2,n_bins2] int32, outside [1] int32 (both or neither; ZEROED BY THE CALLER, the launch ADDS)
 *                         the joint histogram of components (comp_a, comp_b): bin = floor((v - lo) * n_bins2 / (hi - lo))
 *                         in fp64 for lo <= v < hi, counts[bin_a, bin_b]; a structure with either component outside its
 *                         range or non-finite counts once in outside.  LDS integer atomics, one integer vector atomic
 *                         per non-zero slot: exact in any order.
 * Limits as above, 1 <= n_bins2 <= cgv_tica_max_bins2(), lo < hi finite. */
int cgv_tica_max_features(void);
int cgv_tica_max_atoms(void);
int cgv_tica_max_bins2(void);
int cgv_tica_max_components(void);
int cgv_tica_moments_splits(int n_frames, int d, int lag);            /* frame ranges of a call; 0: the call adds nothing */
size_t cgv_tica_moments_workspace_bytes(int n_frames, int d, int lag);
int cgv_tica_moments(const float* xyz, const int32_t* pairs /*[d,2]*/, int n_frames, int n_atoms, int d, int lag,
                     double* sum_x, double* sum_y, double* cxx, double* cyy, double* cxy, void* workspace,
                     size_t workspace_bytes, void* stream);
int cgv_tica_project(const float* xyz, const int32_t* pairs /*[d,2]*/, const double* mean, const double* W /*[d,k]*/,
                     int n_structures, int n_atoms, int d, int k, double* ics /*[n_structures,k]*/, int comp_a, int comp_b,
                     int n_bins2, double lo_a, double hi_a, double lo_b, double hi_b, int32_t* counts, int32_t* outside,
                     void* stream);

/* ---------------------------------------------------------------------------------------
 * K17  superposed RMSD between two sets of structures -- coverage (recall) and precision of a generated ensemble: does
 * every conformation of the data have a generated structure near it, is every generated structure near some conformation
 * of the data?  "Near" is the whole-structure RMSD after optimal superposition.  Nothing in the reference computes it.
 *   a [sa,n_atoms,3], b [sb,n_atoms,3] fp32   the two sets (the same pointer for a set against itself)
 *   sel [m] int32, 1 <= m <= n_atoms          the atoms that count.  An index outside [0, n_atoms) reads atom 0 (the host
 *                                             wrapper refuses such a selection); nothing is read out of bounds.
 *   rmsd^2(i, j) = max(0, G_a[i] + G_b[j] - 2 lambda(i, j)) / m
 * G: the sum of squared coordinates over sel after subtracting their centroid (summed over sel in ascending order);
 * lambda: the largest eigenvalue of the 4 x 4 quaternion key matrix of M = sum_k a~_i[k]^T b~_j[k], i.e. the maximum over
 * PROPER rotations only -- a mirror image is not a superposition.  Coordinates are widened on load, everything after is
 * fp64.  lambda comes from a fixed number of cyclic Jacobi sweeps: degenerate M (one or two atoms, collinear or planar
 * selections, identical structures) is an ordinary input.
 * A structure with a non-finite coordinate inside sel is `bad`: its pairs are NaN in `dense` and enter no minimum.
 *
 * The call MERGES into the caller's running nearest neighbours (initialised by the caller to +inf / -1):
 *   row_min [sa] fp64, row_arg [sa] int32     min over j of rmsd^2(i, j) and the GLOBAL index off_b + j of that column
 *   col_min [sb] fp64, col_arg [sb] int32     min over i and off_a + i
 * keeping the smaller value and, on equal bits, the lower index -- so a caller may cut both sets into chunks, pass each
 * pair of chunks with its offsets, and get the bits of a single call.  same != 0 skips the pairs off_a + i == off_b + j
 * (a set against itself).
 *   dense [sa,sb] fp64 (may be NULL)          every rmsd^2 of this call, overwritten (the diagonal of `same` included)
 * Launches: one thread per structure for centroid, G and bad; grid (tiles of 32 rows, tiles of 32 columns) x 256 threads,
 * a block stages 16 selected atoms of its 64 structures as three fp64 coordinate planes per side in LDS, each wave keeps
 * the nine entries of M for its 16 x 16 pairs as nine accumulators of v_mfma_f64_16x16x4_f64, solves for lambda in
 * registers and the block reduces its 32 x 32 values to per-row and per-column (value, index) partials in the workspace;
 * a last launch merges the partials in ascending tile order.  No [sa,sb] tensor unless `dense` is asked for, no
 * floating-point atomics: the same bits on every run.
 * workspace: cgv_superpose_workspace_bytes(sa, sb) bytes, 8-byte aligned, contents need not survive.
 * Limits: sa, sb <= cgv_superpose_max_structures(), n_atoms <= cgv_superpose_max_atoms(), off + s <= INT32_MAX; beyond a
 * limit the call fails (CGV_E_BADARG) before any launch.  Bound: see DESIGN.md (K17 row). */
int cgv_superpose_max_structures(void);
int cgv_superpose_max_atoms(void);
size_t cgv_superpose_workspace_bytes(int sa, int sb);
int cgv_superpose(const float* a, const float* b, const int32_t* sel /*[m]*/, int sa, int sb, int n_atoms, int m, int off_a,
                  int off_b, int same, double* row_min, int32_t* row_arg, double* col_min, int32_t* col_arg,
                  double* dense /*[sa,sb] or NULL*/, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * K18  Girvan-Newman partition of the bond graph (`-cg_method newman`) -- replaces get_partition
 * (CoarseGrainingVAE/datasets.py:373-385: networkx.community.girvan_newman): remove the live edge of highest betweenness
 * until the graph has n_cgs connected components.
 *   rowptr [n+1], col [2m], edge_id [2m] int32   CSR of the undirected graph over atoms: every edge fills one slot of each
 *                           endpoint's row, edge_id names its undirected edge 0..m-1.  No self loops, no edge twice, col in
 *                           [0, n), edge_id in [0, m): the CALLER guarantees this (cgmap.bond_csr builds it).
 *   edges  [m,2] int32      the endpoints of edge e
 *   alive  [m]   int32      != 0: the edge is still in the graph
 * cgv_newman_betweenness (no reference line of its own: networkx.edge_betweenness_centrality inside girvan_newman): bet [m]
 *   fp64 = sum over ALL sources s of Brandes' dependency of s on the edge (every unordered pair counts twice; networkx
 *   scales the same sums by a constant), over all connected components at once; 0 for an edge that is not alive.
 *   Launches: a grid of cgv_newman_groups(n, groups) workgroups, each running a contiguous range of ceil(n / groups) sources
 *   one after the other (groups = 0: the rule, at most 512) and writing one partial row [m]; then one workgroup adds the
 *   rows in row order.  Path counts and dependencies are fp64, every sum has a fixed order, there is no floating-point
 *   atomic: the same bits on every run, and in both forms.
 * cgv_newman_components (datasets.py:363-371, parition2mapping over nx.connected_components): labels [n] int32 = the lowest
 *   atom index of the atom's component under `alive`; state[0] = number of components, state[1] = 0.  Bead k of the
 *   reference's numbering is the component with the k-th smallest label.
 * cgv_newman_partition (datasets.py:373-385): enqueues `removals` rounds of three launches on `stream` --
 *   betweenness; reduce + choose + remove: among the live edges whose betweenness is within a relative 1e-9 of the maximum
 *   the one with the lowest (min(u,v), max(u,v)) goes (for edges listed in sorted order: networkx's first maximum whenever
 *   its values tie exactly), alive[e] = 0, log[state[1]++] = e; components: a BFS from one endpoint of the removed edge,
 *   and when the other is not reached both sides are relabelled and state[0] goes up.
 *   Every launch returns at once when state[0] >= n_cgs, so the caller may enqueue a batch and read state[0] (4 bytes)
 *   once per batch; rounds enqueued after the end change nothing.  Needs labels / state from cgv_newman_components (or
 *   from earlier rounds) and log [m] int32.  No launch waits for another workgroup.
 * form: CGV_NEWMAN_RESIDENT -- a workgroup's state (level, sigma, delta per atom, its partial row, the live adjacency) in
 *   LDS, needs cgv_newman_resident_fits(n, m); CGV_NEWMAN_STREAMED -- the same state in the workspace.
 * workspace: cgv_newman_workspace_bytes(n, m, form, groups) bytes, 256-byte aligned; the same form and groups in every call
 *   that shares it; contents need not survive between calls.
 * Limits: n <= 2^20, m <= 2^22; beyond them the calls fail (CGV_E_BADARG) before any launch. */
#define CGV_NEWMAN_RESIDENT 1
#define CGV_NEWMAN_STREAMED 2
int cgv_newman_resident_fits(int n, int m);
int cgv_newman_groups(int n, int groups);
size_t cgv_newman_workspace_bytes(int n, int m, int form, int groups);
int cgv_newman_betweenness(const int32_t* rowptr, const int32_t* col, const int32_t* edge_id, const int32_t* alive, int n, int m,
                           int form, int groups, double* bet /*[m]*/, void* workspace, size_t workspace_bytes, void* stream);
int cgv_newman_components(const int32_t* rowptr, const int32_t* col, const int32_t* edge_id, const int32_t* edges /*[m,2]*/,
                          const int32_t* alive, int n, int m, int form, int groups, int32_t* labels /*[n]*/,
                          int32_t* state /*[2]*/, void* workspace, size_t workspace_bytes, void* stream);
int cgv_newman_partition(const int32_t* rowptr, const int32_t* col, const int32_t* edge_id, const int32_t* edges /*[m,2]*/,
                         int32_t* alive, int32_t* labels /*[n]*/, int32_t* state /*[2]*/, int32_t* log /*[m]*/, int n, int m,
                         int n_cgs, int removals, int form, int groups, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * K19  baseline models (`run_baseline -model linear | equilinear | mlp`) -- replaces the optimiser loop of
 * scripts/run_baseline.py:121-176 (losses 86-92, 147-149; torch.optim.Adam 304) on Baseline (CoarseGrainingVAE/baseline.py:
 * 8-36) and EquiLinear (baseline.py:387-443) under the fixed pooler CGpool (diffpoolvae.py:105-195: cg = bead means), and
 * the loss of the MLP (baseline.py:109-147).  Both linear models are one matrix over feature vectors of the bead means:
 *   dx[b,a,:] = sum_c P(a,c) U[b,c,:]
 *   CGV_BASELINE_LINEAR      B [K,n], P(a,c) = B[c,a], C = K; U[b,c] = cg[b,c] - mean_atoms(xyz[b]);
 *                            recon = dx against xyz - mean_atoms(xyz)
 *   CGV_BASELINE_EQUILINEAR  B [n, K knn], P(a,c) = B[a,c], C = K knn; U[b, i knn + (c-1)] = cg[b,c] - cg[b,i], c = 1..knn
 *                            (c is a bead index, as in the reference: it takes nonzero() of the SORTED distances, so the
 *                            pair's second index is the rank position used as a bead id); recon[b,a] = cg[b,m(a)] -
 *                            mean_{a' in bead m(a)} dx[b,a'] + dx[b,a] against xyz.  1 <= knn <= K - 1.
 *   loss_recon = mean over b n 3 of (recon - target)^2; loss_dist = mean over (b, e) of (|recon_i - recon_j| - |x_i - x_j|)^2
 *   over the hyperedges e = (i, j); loss = loss_recon + gamma loss_dist; Adam (bias correction, no weight decay) on B.
 * Two deliberate deviations from the reference, in cgv_baseline_steps and cgv_baseline_loss alike: a hyperedge whose
 * RECONSTRUCTED length is exactly 0 contributes 0 to the gradient (reference: NaN), and an empty hyperedge list gives
 * loss_dist = 0 (reference: NaN).
 *   B, mB, vB               the parameter and its Adam moments in the reference's layout, updated in place (mB, vB may be
 *                           NULL in forward mode)
 *   frames [n_frames,n,3]   as they are (not centred)
 *   order, order_len, n_train, batch, step0, steps      the schedule, exactly as in cgv_cgae_steps: the last, partial batch
 *                           of an epoch is kept and its means divide by its own counts; Adam's step count is step + 1
 *   mapping [n] int32 in [0,K), bead_sizes [K] int32 (> 0: the CALLER guarantees it), edges [E,2] int32 hyperedges of the
 *   molecule shared by all frames (indices outside [0,n) are clamped; E may be 0)
 *   loss_log [steps,2]      (loss_recon, loss_dist) of every step of this call
 *   probe  optional         of the call's LAST step: xyz_recon [batch,n,3], then (train mode) the gradient in B's layout
 *   mode   CGV_BASELINE_TRAIN, or CGV_BASELINE_FORWARD: forward and losses only, B and the moments untouched
 * form: CGV_BASELINE_RESIDENT -- B, both moments, the bead means and U in the LDS of the one workgroup that runs the call,
 *   needs cgv_baseline_resident_fits(kind, n, C, batch) (3 n C + 6 batch (3 C + 1) + 32 floats within 160 KB: the small per-batch arrays are doubles);
 *   CGV_BASELINE_GLOBAL -- the same single-workgroup loop on the caller's arrays in place, small arrays in the workspace.
 *   Every sum has a fixed order and there is no floating-point atomic: a call of `steps` steps equals `steps` calls of one,
 *   a repeated call gives the same bits, and the two forms give the same bits.
 * Cap: n C, batch n, batch C, batch E and 2 E below 2^24 and K <= n; beyond it the calls fail (CGV_E_BADARG) before any
 *   launch.  The global form is correct at every size below the cap.
 * workspace: cgv_baseline_workspace_bytes(...), 256-byte aligned, contents need not survive between calls.
 * cgv_baseline_loss: for xyz_recon, xyz [b,n,3] (the MLP's output and its target) losses[0] = loss_recon, losses[1] =
 *   loss_dist and grad [b,n,3] = d(loss_recon + gamma loss_dist) / d xyz_recon, one launch of b blocks; the blocks' loss
 *   partials are added in frame order by the last block to arrive (no floating-point atomic: the same bits on every run).
 *   workspace: cgv_baseline_loss_workspace_bytes(b, n, E) bytes whose first 256 are ZERO before the first call (every call
 *   leaves them zero); one call at a time per workspace.  Cap: b <= 65535, b n and b E below 2^24, n E below 2^28. */
#define CGV_BASELINE_LINEAR 1
#define CGV_BASELINE_EQUILINEAR 2
#define CGV_BASELINE_RESIDENT 1
#define CGV_BASELINE_GLOBAL 2
#define CGV_BASELINE_TRAIN 0
#define CGV_BASELINE_FORWARD 1
int cgv_baseline_resident_fits(int kind, int n_atoms, int C, int batch);
size_t cgv_baseline_workspace_bytes(int kind, int n, int K, int knn, int batch, int E, int form);
int cgv_baseline_steps(int kind, int form, int mode, float* B, float* mB, float* vB, const float* frames, int n_frames,
                       const int32_t* order, int64_t order_len, int n_train, int batch, int n, int K, int knn,
                       const int32_t* mapping, const int32_t* bead_sizes, const int32_t* edges /*[E,2]*/, int E, int64_t step0,
                       int steps, float gamma, double lr, double beta1, double beta2, double eps, float* loss_log /*[steps,2]*/,
                       float* probe, void* workspace, size_t workspace_bytes, void* stream);
size_t cgv_baseline_loss_workspace_bytes(int b, int n, int E);
int cgv_baseline_loss(const float* xyz_recon, const float* xyz, const int32_t* edges /*[E,2]*/, int b, int n, int E, float gamma,
                      float* losses /*[2]*/, float* grad /*[b,n,3]*/, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * K20  contact maps of an ensemble -- which atoms (or groups of atoms: beads, residues) touch, how compact a structure is,
 * and whether it has the contacts the data has: contact probability maps, the fraction of native contacts Q and the
 * radius of gyration.  Nothing in the reference computes them.
 *   xyz [n_structures,n_atoms,3] fp32
 *   sel [m] int32, 1 <= m <= n_atoms          the atoms that count, in any order; all indices below are positions in sel.
 *                                             An index outside [0, n_atoms) reads atom 0 (the host wrapper refuses such a
 *                                             selection); nothing is read out of bounds.
 *   excluded [m, ceil(m/32)] uint32           bit (j & 31) of word [i][j >> 5]: the pair (i, j) never counts (bonded
 *                                             neighbours).  The CALLER keeps it symmetric; the diagonal never counts.
 *   native (may be NULL)                      the same layout (cgv_contact_group_counts: [n_groups, ceil(n_groups/32)] over
 *                                             groups): the pairs whose contacts n_native counts
 *   cutoff2 fp32 >= 0                         the squared cutoff
 * A pair (i, j), i != j, not excluded, is in contact in structure s iff (dx*dx + dy*dy) + dz*dz < cutoff2, fp32 with
 * every operation individually rounded (csrc/sq_dist.h: sq_dist2) and strict <: a host that restates the sum gets every
 * integer below exactly.
 *   counts [m,m] int32                        the structures in which (i, j) is in contact are ADDED to both [i][j] and
 *                                             [j][i] (the diagonal is not touched): a caller cuts a long ensemble into
 *                                             launches and zeroes the table once.  Total structures < 2^31: the CALLER's.
 *   n_contacts [n_structures] int32           overwritten: unordered pairs in contact in structure s
 *   n_native   [n_structures] int32           overwritten: those of them that are in `native` (0 without one)
 *   rg2 [n_structures] fp64                   overwritten: mean over sel of |x - centroid|^2, fp64 from widened
 *                                             coordinates, two passes, fixed summation tree (may be NULL in the group call)
 *   bad [n_structures] int32                  overwritten: 1 for a structure with a non-finite coordinate inside sel.  It
 *                                             adds nothing to counts, has n_contacts = n_native = -1 and rg2 = NaN.
 * cgv_contact_group_counts: sel is sorted so that the atoms of group g are the positions group_start[g] ..
 *   group_start[g + 1] - 1 (group_start [n_groups + 1] int32, ascending from 0 to m).  Groups A != B are in contact in
 *   structure s iff ANY non-excluded pair (a in A, b in B) is; group_counts [n_groups,n_groups] int32 is added to like
 *   counts, n_contacts / n_native count pairs of groups.  (Not derivable from counts: the "any" is per structure.)
 * Launches: one wave per structure gathers sel into a packed copy [n_structures, m] float4 in the workspace and computes
 *   rg2 and bad (a bad structure's copy is NaN: in contact with nothing).  cgv_contact_counts: grid (tiles of 128 columns,
 *   tiles of 64 rows, slices of the structure axis) x 256 threads over the tiles that hold a pair i < j; a thread keeps the
 *   32 counters of its row and its wave's 32 columns in registers, 8 structures at a time pass through 24 KB of LDS; the
 *   slices -- as many as bring the grid to 1024 blocks, of at least 64 structures -- meet in integer atomicAdd.
 *   cgv_contact_group_counts: grid (n_groups, n_groups, slices) x one wave, 64 structures per pass.
 *   Integer sums do not depend on their order and rg2 uses no atomic: the same bits on every run.
 * workspace: cgv_contact_workspace_bytes(n_structures, m) bytes, 16-byte aligned, contents need not survive.
 * Limits: m <= cgv_contact_max_atoms(), n_structures <= cgv_contact_max_structures() per launch, n_groups <= min(m, 4096);
 * beyond a limit the call fails (CGV_E_BADARG) before any launch.  Bound: see DESIGN.md (K20 row). */
int cgv_contact_max_atoms(void);
int cgv_contact_max_structures(void);
size_t cgv_contact_workspace_bytes(int n_structures, int m);
int cgv_contact_counts(const float* xyz, const int32_t* sel /*[m]*/, const uint32_t* excluded, const uint32_t* native /*or NULL*/,
                       int n_structures, int n_atoms, int m, float cutoff2, int32_t* counts /*[m,m]*/, int32_t* n_contacts,
                       int32_t* n_native, double* rg2, int32_t* bad, void* workspace, size_t workspace_bytes, void* stream);
int cgv_contact_group_counts(const float* xyz, const int32_t* sel /*[m]*/, const int32_t* group_start /*[n_groups+1]*/,
                             const uint32_t* excluded, const uint32_t* native /*or NULL*/, int n_structures, int n_atoms, int m,
                             int n_groups, float cutoff2, int32_t* group_counts /*[n_groups,n_groups]*/, int32_t* n_contacts,
                             int32_t* n_native, double* rg2 /*or NULL*/, int32_t* bad, void* workspace, size_t workspace_bytes,
                             void* stream);

/* ---------------------------------------------------------------------------------------
 * K21  superpose an ensemble onto a target and accumulate its mean structure and per-atom fluctuation (RMSF) -- how much
 * an ensemble moves.  Nothing in the reference superposes anything.
 *   xyz [n_structures,n_atoms,3] fp32         the structures
 *   sel [m] int32, 1 <= m <= n_atoms          the atoms the superposition is fitted on.  An index outside [0, n_atoms) is
 *                                             ignored and an atom named twice counts once (the host wrapper refuses both).
 *   ref [n_atoms,3] fp64                      the target
 * Per structure: structure and target are centred on the centroid of their selected atoms; M = sum over sel of a~^T b~ in
 * fp64 on exactly widened coordinates; the PROPER rotation R that maximises sum b~ . R a~ from the eigenvector of the
 * largest eigenvalue of the quaternion key matrix (csrc/superpose_rot.h: the Jacobi sweeps of K17 with the rotations
 * accumulated, a deterministic rule for the sign and inside a degenerate eigenspace; a mirror image is never a solution);
 * y = R a~ for EVERY atom.  The call MERGES (adds) into the caller's accumulators, so a caller may chunk:
 *   sum [n_atoms,3] fp64                      += y of every good structure (the centred frame of the target)
 *   dev2 [n_atoms] fp64                       += |y - b~|^2
 *   n_good [1] int32                          += structures that are not bad
 * and overwrites, per structure,
 *   rmsd2 [n_structures] fp64                 max(0, G_a + G_b - 2 lambda) / m over the selection; NaN for a bad structure
 *   bad [n_structures] int32                  1 when ANY coordinate of the structure is not finite: it contributes nothing
 *   aligned [n_structures,n_atoms,3] fp32     (may be NULL) y, rounded; NaN for a bad structure
 * form: 0 the rule (cgv_align_wave_fits(n_atoms): a wave owns a structure, else a block of 256 threads does), 1 / 2 force
 * either.  Two launches: groups of threads own contiguous ranges of structures (at least 4; as many ranges as bring the
 * grid to 4096 waves / 512 blocks), a thread owns atoms and keeps their accumulators in registers, the selection is a bit
 * mask in LDS so every structure is read once; reductions are fixed trees; a second launch adds the ranges' partial sums
 * in ascending order.  No [S,n,3] fp64 intermediate, no floating-point atomics: the order of every addition is a function
 * of (n_structures, n_atoms, m, form) alone -- the same bits on every run.
 * workspace: cgv_align_workspace_bytes(n_structures, n_atoms, form) bytes, 8-byte aligned, contents need not survive.
 * Limits: n_atoms <= cgv_align_max_atoms(), n_structures <= cgv_align_max_structures() per launch; beyond a limit the call
 * fails (CGV_E_BADARG) before any launch.  Bound: see DESIGN.md (K21 row). */
int cgv_align_max_atoms(void);
int cgv_align_max_structures(void);
int cgv_align_wave_fits(int n_atoms);
size_t cgv_align_workspace_bytes(int n_structures, int n_atoms, int form);
int cgv_align_accumulate(const float* xyz, const int32_t* sel /*[m]*/, const double* ref /*[n_atoms,3]*/, int n_structures,
                         int n_atoms, int m, int form, double* sum /*[n_atoms,3]*/, double* dev2 /*[n_atoms]*/, int32_t* n_good,
                         double* rmsd2, int32_t* bad, float* aligned /*or NULL*/, void* workspace, size_t workspace_bytes,
                         void* stream);

/* ---------------------------------------------------------------------------------------
 * K15b  the internal-coordinate VALUES that K15 bins: values [n_structures,n_features] fp64 of the feature records
 * (feat, kind: as cgv_internal_hist), through the same device function and the same operation order (no FMA contraction).
 * An invalid item (K15's rule) is written as NaN and ADDS one to n_invalid [1] int32 (zeroed by the caller).  One launch,
 * one thread per item.  Limits: n_features / n_atoms as K15, n_atoms >= 1, n_structures * n_features <= 2^36. */
int cgv_internal_values(const float* xyz, const int32_t* feat /*[n_features,4]*/, const int32_t* kind /*[n_features]*/,
                        int n_structures, int n_atoms, int n_features, double* values, int32_t* n_invalid, void* stream);

/* ---------------------------------------------------------------------------------------
 * K22  the sums of a Gaussian kernel density estimate -- the numbers behind the reference's kernel_density_plot
 * (CoarseGrainingVAE/plots.py:61-84: scipy.stats.gaussian_kde on a 300 x 300 grid).  For n_planes independent planes:
 *   samples [n_planes,n_samples,d] fp32, points [n_planes,n_points,d] fp32, d = 1 or 2
 *   period  [n_planes,d] fp32 or NULL         0 (or less): the axis is not periodic.  NULL: no axis of any plane is.
 *   sums    [n_planes,n_points] fp64          sums[p,m] = sum_i exp2(-|points[p,m] - samples[p,i]|^2), OVERWRITTEN
 *   n_skipped [n_planes] int32                non-finite samples of the plane (they add no term), OVERWRITTEN
 * On a periodic axis a difference is reduced to its minimum image, delta - period * rint(delta * (1 / period)), before
 * squaring.  The caller has centred, whitened and scaled the coordinates by sqrt(log2(e) / 2): the kernel knows nothing
 * of bandwidths.  fp32 differences, squares and v_exp_f32 of 64 - |delta|^2, scaled back by 2^-64 in fp64 at the end
 * (terms with |delta|^2 > 190 are flushed to zero: nothing that counts in a sum of N 2^-126 or more); a point's
 * terms are added in fp32 within a stage of at most 1024 samples, in sample order, and the stages in fp64.  A non-finite
 * point gives NaN.  n_samples = 0 gives zeros, n_points = 0 only counts; nothing is read out of bounds.
 * Two launches: grid (tiles of 1024 points, `splits` contiguous sample ranges, planes) x 256 threads, a thread owns four
 * points in registers and every lane reads a stage's samples from LDS as broadcasts; the second launch adds the ranges'
 * fp64 partial sums in ascending order.  splits: 0 = cgv_kde_splits(n_planes, n_samples, n_points), a function of the
 * three sizes alone, else 1 .. cgv_kde_max_splits().  No floating-point atomics: the same bits on every call.
 * workspace: cgv_kde_workspace_bytes(n_planes, n_points, splits actually used) bytes, 8-byte aligned, contents need not
 * survive.  Limits: cgv_kde_max_planes / _samples / _points(), n_planes * n_points <= 2^30; beyond a limit the call fails
 * (CGV_E_BADARG) before any launch.  Bound: see DESIGN.md (K22 row). */
int cgv_kde_max_planes(void);
int cgv_kde_max_samples(void);
int cgv_kde_max_points(void);
int cgv_kde_max_splits(void);
int cgv_kde_splits(int n_planes, int n_samples, int n_points);
size_t cgv_kde_workspace_bytes(int n_planes, int n_points, int splits);
int cgv_kde_sums(const float* samples, const float* points, const float* period /*or NULL*/, int n_planes, int n_samples,
                 int n_points, int d, int splits, double* sums, int32_t* n_skipped, void* workspace, size_t workspace_bytes,
                 void* stream);

/* ---------------------------------------------------------------------------------------
 * K23  solvent-accessible surface area of an ensemble (Shrake-Rupley) -- which atoms a structure turns to the solvent:
 * for every structure and every selected atom, how many of n_points points on the atom's probe-inflated sphere lie inside
 * no other selected atom's inflated sphere.  Nothing in the reference computes it.  Lengths in Angstrom.
 *   xyz [n_structures,n_atoms,3] fp32
 *   sel [m] int32, 1 <= m <= n_atoms          the molecule: the atoms probed and the only occluders, in any order; all
 *                                             indices below are positions in sel.  An index outside [0, n_atoms) reads
 *                                             atom 0 (the host wrapper refuses such a selection); nothing is read out of
 *                                             bounds.
 *   r [m] fp32                                the inflated radius of a selected atom, fp32(fp32(R) + fp32(probe)): the
 *                                             CALLER's sum.  r2_j = r_j * r_j, one rounded fp32 product.
 *   u [n_points,3] fp32                       points of the unit sphere, the CALLER's (golden spiral, built in fp64 and
 *                                             rounded once)
 *   cls [m] int32 in [0, n_classes)           the class of a selected atom (a value outside counts as class 0)
 * Point k of atom i is c_i + r_i * u_k per component, the product rounded, then the sum (no fma).  It is buried iff some
 * position j != i of sel has (dx*dx + dy*dy) + dz*dz < r2_j for its difference to c_j, fp32 with every operation
 * individually rounded (csrc/sq_dist.h: sq_dist2) and strict <; j != i is by position, not by coordinates.  count[s,i] is
 * the number of points of atom i that are not buried, 0 .. n_points: a host that restates the arithmetic gets every integer
 * below exactly, and the area of an atom is the host's 4 pi r_i^2 count / n_points -- no floating-point result leaves the
 * device.
 *   counts [n_structures,m] int32 or NULL     overwritten: count[s,i]
 *   class_counts [n_structures,n_classes] int32   overwritten: the sum of count[s,i] over the atoms of a class
 *   atom_sum, atom_sumsq [m] int64            count and count^2 of this call's good structures are ADDED: a caller cuts a
 *                                             long ensemble into launches and zeroes them once
 *   bad [n_structures] int32                  overwritten: 1 for a structure with a non-finite coordinate inside sel.  Its
 *                                             rows of counts and class_counts are -1 and it enters no sum.
 * Launches: one wave per structure gathers sel into a packed copy [n_structures, m] float4 (x, y, z, r2) in the workspace
 *   and writes bad and a flag per structure; then grid (structures x atom ranges, at most 1024 blocks that loop) x 256
 *   threads: a block stages a structure's packed atoms and the sphere points in LDS, a wave owns atoms in turn, compacts the
 *   occluders that pass a pre-filter on |c_i - c_j| into a list in LDS (capacity m - 1), its lanes own points and walk the
 *   list until every live point of the wave is buried.  The pre-filter is a proven superset of the atoms that can bury a
 *   point for |coordinates| <= 4096 (derivation: csrc/sasa.hip); a structure beyond that takes every j != i and is not bad.
 *   The atoms of a structure are split over several blocks when the structures alone would leave CUs idle.  Integer sums
 *   meet in atomicAdd, whose order does not matter: the same bits on every call, however the structures are cut.
 * workspace: cgv_sasa_workspace_bytes(n_structures, m, n_points) bytes (0 beyond a limit), 16-byte aligned, contents need
 *   not survive.
 * Limits: m <= cgv_sasa_max_atoms() (4096: a structure's atoms, its lists and sums live in the 160 KB of LDS of a CU),
 *   n_points <= cgv_sasa_max_points(), n_classes <= cgv_sasa_max_classes(), n_structures <= cgv_sasa_max_structures() per
 *   launch; beyond a limit the call fails (CGV_E_BADARG) before any launch.  Bound: see DESIGN.md (K23 row). */
int cgv_sasa_max_atoms(void);
int cgv_sasa_max_points(void);
int cgv_sasa_max_classes(void);
int cgv_sasa_max_structures(void);
size_t cgv_sasa_workspace_bytes(int n_structures, int m, int n_points);
int cgv_sasa_counts(const float* xyz, const int32_t* sel /*[m]*/, const float* r /*[m]*/, const float* u /*[n_points,3]*/,
                    const int32_t* cls /*[m]*/, int n_structures, int n_atoms, int m, int n_points, int n_classes,
                    int32_t* counts /*[S,m] or NULL*/, int32_t* class_counts /*[S,n_classes]*/, int64_t* atom_sum /*[m]*/,
                    int64_t* atom_sumsq /*[m]*/, int32_t* bad /*[S]*/, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * K24  clustering of an ensemble by superposed RMSD (Daura et al., "GROMOS": the default of `gmx cluster -method gromos`)
 * -- which conformational states the data has: the dense squared RMSDs of K17 become a bit-packed neighbour matrix, and
 * the greedy loop (the structure with most neighbours becomes a centre, it and its neighbours leave, repeat) runs on the
 * device, so no [S,S] fp64 tensor reaches the host.  Nothing in the reference computes it.
 *   c2 = double(cutoff) * double(cutoff), the CALLER's product.  All comparisons are exact.
 *   For structures p < q: adj(p, q) = adj(q, p) = (d2(p, q) <= c2), d2(p, q) the value cgv_superpose writes to `dense` for
 *   row p, column q of the set against itself.  Only the UPPER triangle decides (the transposed pair may differ in its last
 *   bits; the graph must be symmetric).  adj(p, p) = 1 iff p is good: dense[p, p] is not NaN.  NaN compares false: a bad
 *   structure has an empty row and an empty column.
 *   bits [S, W] uint64, W = ceil(S / 64): bit (q & 63) of word q >> 6 of row p is adj(p, q); bits at columns >= S are 0.
 *
 * cgv_cluster_pack: one dense rectangle of a pair of chunks of the set.
 *   dense [sa,sb] fp64                        cgv_superpose's `dense` for rows off_a .. off_a + sa, columns off_b .. off_b + sb
 *   off_a <= off_b, both multiples of 64; the chunks are the same one (off_a == off_b, sa == sb) or apart (off_a + sa <=
 *   off_b); only the chunk that ends at n_structures may be no multiple of 64 long.
 *   It writes every word of `bits` the rectangle decides: rows off_a.., words off_b / 64.. (in the diagonal chunk: from
 *   dense[min(i, j), max(i, j)]), and, mirrored, rows off_b.., words off_a / 64...  A caller that passes every pair of
 *   chunks with off_a <= off_b once has written every word exactly once; the result does not depend on the chunk size.
 *   Launch: grid (column tiles, row tiles) x 256 threads, a 64 x 64 tile per block: a wave reads 64 consecutive doubles of
 *   a row, ballots the comparison, one lane stores the word and keeps it in LDS; the mirrored words are ballots over the 64
 *   staged words, so every read of `dense` is coalesced.  No atomics.
 * cgv_cluster_gromos: the clustering of a finished bit matrix.
 *   good [W] uint64 or NULL                   the structures that take part (a bit mask); NULL: those with their diagonal
 *                                             bit.  Bits at positions >= n_structures are ignored.
 *   alive starts as the good structures, count[i] = popcount(row_i & alive).  An iteration k: the centre c is the alive
 *   structure of largest count, lowest index on ties; its members are row_c & alive plus c itself, whatever its diagonal
 *   bit says; they get label k and leave alive; for every removed r the counts of its alive neighbours are decremented
 *   (the matrix is symmetric; no row is recounted).  At most n_structures iterations, each removes at least its centre: a
 *   matrix that is not symmetric gives other clusters, never a hang.
 *   label [S] int32                           overwritten: the cluster of a structure, -1 for one that is not good
 *   centre [S], size [S] int32                overwritten: the first *n_clusters entries are the centre and the number of
 *                                             members of a cluster, in the order found; the rest is -1 / 0
 *   n_clusters [1] int32                      overwritten
 *   Launch: ONE workgroup of 1024 threads with alive, the members of the iteration, the counts and the reduction scratch in
 *   LDS (dynamic, 272 bytes per 64 structures + 144); decrements are integer LDS atomics.  Integers only: the same bits
 *   on every call.
 * cgv_cluster_workspace_bytes(n_structures, chunk): the bit matrix (128 MiB at the limit) followed by one dense chunk of
 *   `chunk` rounded up to 64, squared, doubles; 0 beyond a limit.
 * Limits: n_structures <= cgv_cluster_max_structures() (32768: what the 160 KB of LDS of a CU hold); beyond it the calls
 *   fail (CGV_E_BADARG) before any launch.  See DESIGN.md (K24 row). */
int cgv_cluster_max_structures(void);
size_t cgv_cluster_workspace_bytes(int n_structures, int chunk);
int cgv_cluster_pack(const double* dense /*[sa,sb]*/, int sa, int sb, int off_a, int off_b, int n_structures, double c2,
                     uint64_t* bits /*[S,W]*/, void* stream);
int cgv_cluster_gromos(const uint64_t* bits /*[S,W]*/, const uint64_t* good /*[W] or NULL*/, int n_structures,
                       int32_t* label /*[S]*/, int32_t* centre /*[S]*/, int32_t* size /*[S]*/, int32_t* n_clusters /*[1]*/,
                       void* stream);

/* ---------------------------------------------------------------------------------------
 * K25  hydrogen bonds of an ensemble (Baker-Hubbard, intramolecular) -- which donor hydrogens point at which acceptors:
 * how often every pair (donor hydrogen, acceptor) is bonded over the structures, per structure the number of bonds and of
 * native bonds, and on request every bond of every structure as a bit.  Nothing in the reference computes it.  Lengths in
 * Angstrom.
 *   xyz [n_structures,n_atoms,3] fp32
 *   don_h, don_d [n_hydrogens] int32          a donor hydrogen and the heavy atom it is bonded to: the CALLER's tables
 *   acc [n_acceptors] int32                   the acceptors.  An index outside [0, n_atoms) reads atom 0 (the host wrapper
 *                                             builds the tables itself); nothing is read out of bounds.
 *   excluded [n_hydrogens,W] uint64, W = ceil(n_acceptors / 64): bit (a & 63) of word a >> 6 of row h: the pair (h, a) never
 *                                             counts (A is D, A is bonded to D, or the caller says so).  Bits past
 *                                             n_acceptors are ignored.
 *   native [n_hydrogens,W] uint64 or NULL     the pairs n_native counts, in the same layout
 * A pair that is not excluded is bonded in a structure iff, in fp32 with every operation individually rounded (no fma),
 *   d2 = sq_dist2(A, H), l2 = sq_dist2(D, H)  ((dx*dx + dy*dy) + dz*dz, csrc/sq_dist.h),
 *   dot = (ux*vx + uy*vy) + uz*vz with u = D - H and v = A - H, and
 *   d2 < cutoff2  and  dot < 0  and  dot*dot > (c2 * l2) * d2.
 * cutoff2 is the CALLER's fp32(cutoff) * fp32(cutoff), c2 the CALLER's fp32(cos(angle)^2) of the least D-H...A angle, which
 * must lie in [90, 180) degrees for the test to mean cos(D-H-A) < cos(angle).  A host that restates the arithmetic gets
 * every integer below exactly; no floating-point result leaves the device.
 *   pair_counts [n_hydrogens,n_acceptors] int64   ADDED to: in how many good structures of this call the pair is bonded; a
 *                                             caller cuts a long ensemble into launches and zeroes it once
 *   n_hbonds [n_structures] int32             overwritten: the bonds of a structure
 *   n_native [n_structures] int32             overwritten: those of them in `native` (0 when native is NULL)
 *   bad [n_structures] int32                  overwritten: 1 for a structure with a non-finite coordinate in an atom of
 *                                             don_h, don_d or acc.  Its n_hbonds and n_native are -1, it enters no sum.
 *   bits [n_structures,n_hydrogens,W] uint64 or NULL   overwritten: bit (a & 63) of word a >> 6 is set iff (h, a) is bonded;
 *                                             bits past n_acceptors are 0, the rows of a bad structure are 0
 * Launches: one wave per structure gathers the table atoms into a packed copy [n_structures, 2 n_hydrogens + n_acceptors]
 *   float4 in the workspace (NaN for a bad structure) and writes bad; then grid (W, row tiles of cgv_hbond_row_tile()
 *   hydrogens, slices of the structure axis) x 256 threads: a lane owns an acceptor, a wave 8 rows whose counters its lanes
 *   keep in registers; cgv_hbond_chunk() structures at a time go through LDS; the wave's ballot of the test is the word of
 *   `bits`.  Integer sums meet in atomicAdd: the same bits on every call, however the structures are cut.
 * workspace: cgv_hbond_workspace_bytes(n_structures, n_hydrogens, n_acceptors) bytes (0 beyond a limit), 16-byte aligned,
 *   contents need not survive.
 * Limits: 1 <= n_hydrogens <= cgv_hbond_max_hydrogens(), 1 <= n_acceptors <= cgv_hbond_max_acceptors(), n_structures <=
 *   cgv_hbond_max_structures() per launch; beyond a limit, and for a cutoff2 or c2 that is no number of its range, the call
 *   fails (CGV_E_BADARG) with its reason before any launch.  See DESIGN.md (HB row). */
int cgv_hbond_max_structures(void);
int cgv_hbond_max_hydrogens(void);
int cgv_hbond_max_acceptors(void);
int cgv_hbond_row_tile(void);
int cgv_hbond_chunk(void);
size_t cgv_hbond_workspace_bytes(int n_structures, int n_hydrogens, int n_acceptors);
int cgv_hbond_counts(const float* xyz, const int32_t* don_h /*[nH]*/, const int32_t* don_d /*[nH]*/, const int32_t* acc /*[nA]*/,
                     const uint64_t* excluded /*[nH,W]*/, const uint64_t* native /*[nH,W] or NULL*/, int n_structures,
                     int n_atoms, int n_hydrogens, int n_acceptors, float cutoff2, float c2, int64_t* pair_counts /*[nH,nA]*/,
                     int32_t* n_hbonds /*[S]*/, int32_t* n_native /*[S]*/, int32_t* bad /*[S]*/,
                     uint64_t* bits /*[S,nH,W] or NULL*/, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * K26  secondary structure of an ensemble (DSSP, Kabsch & Sander 1983) -- which residues are helix, strand, turn or bend:
 * per structure the class of every residue and the residues of every class, and over the structures how often every
 * residue is in every class.  Backbone heavy atoms only (the amide H is virtual).  Nothing in the reference computes it.
 * Lengths in Angstrom.
 *   xyz [n_structures,n_atoms,3] fp32
 *   res [n_residues,4] int32                  N, CA, C, O of residue r, the residues in chain order: the CALLER's tables
 *   prev [n_residues,2] int32                 the carbonyl C' bonded to N(r) and its O'; -1, -1: the residue has no amide
 *                                             hydrogen and never donates (a chain start, a proline)
 *   link [n_residues] int32                   1 iff C(r) is bonded to N(r+1); link[n_residues - 1] is taken as 0.
 *                                             An atom index outside [0, n_atoms) reads atom 0 (the host wrapper builds the
 *                                             tables itself); nothing is read out of bounds.
 * All of it in fp32 with every operation individually rounded (no fma; sqrtf and / correctly rounded), every test written so
 * that a NaN fails it:
 *   virtual hydrogen  w = C' - O',  l = sqrtf((wx*wx + wy*wy) + wz*wz),  H_k = N_k + w_k / l
 *   hb[i][j]          C=O of i accepts from N-H of j: j has an H, j != i, j != i + 1, sq_dist2(CA_i, CA_j) < 81 and e < -0.5
 *                     with e = 27.888 * (((1/rON + 1/rCH) - 1/rOH) - 1/rCN), r = sqrtf(sq_dist2), and e = -9.9 when one of the
 *                     four squared distances is < 0.25
 *   cont(a, b)        link[a .. b-1] are all 1
 *   turn_n(i)         hb[i][i+n] and cont(i, i+n), n = 3, 4, 5
 *   bridge (i, j)     |i-j| >= 3, i+-1 and j+-1 exist, cont(i-1, i+1), cont(j-1, j+1);
 *                     par = (hb[i-1][j] & hb[j][i+1]) | (hb[j-1][i] & hb[i][j+1]),
 *                     anti = (hb[i][j] & hb[j][i]) | (hb[i-1][j+1] & hb[j-1][i+1]);  in a ladder when the same type also holds
 *                     at (i+1, j+1) or (i-1, j-1) (par), at (i+1, j-1) or (i-1, j+1) (anti)
 *   bend(i)           cont(i-2, i+2), u = CA_i - CA_{i-2}, v = CA_{i+2} - CA_i: uu > 0, vv > 0 and (dot <= 0 or
 *                     dot*dot < (c2*uu)*vv), c2 = cgv_dssp_bend_c2() = fp32(cos(70 degrees)^2)
 *   classes, each stage reading only finished earlier ones, code = index into "HBEGITS-":
 *                     H  i..i+3 where turn_4(i-1) & turn_4(i);  E  not H, a bridge that is in a ladder;  B  not H, a bridge
 *                     but none in a ladder;  G  i..i+2 where turn_3(i-1) & turn_3(i), none of the three H E B;  I  i..i+4
 *                     likewise for n = 5, none of the five H E B G;  T  unassigned and turn_n(i-k), 1 <= k < n;  S  unassigned
 *                     and bend;  -  otherwise
 * A host that restates the arithmetic gets every integer below exactly; no floating-point result leaves the device.
 *   class_counts [n_residues,8] int64         ADDED to: in how many good structures of this call residue r has class c; a
 *                                             caller cuts a long ensemble into launches and zeroes it once
 *   n_class [n_structures,8] int32            overwritten: the residues of every class (a row sums to n_residues)
 *   bad [n_structures] int32                  overwritten: 1 for a structure with a non-finite coordinate in an atom of res
 *                                             or prev.  Its n_class row is -1, its codes are 255, its hb_bits 0; it enters
 *                                             no sum.
 *   codes [n_structures,n_residues] uint8 or NULL   overwritten: the class of every residue
 *   hb_bits [n_structures,n_residues,W] uint64 or NULL, W = ceil(n_residues / 64)   overwritten: bit (j & 63) of word j >> 6 of
 *                                             row i is hb[i][j]; bits past n_residues are 0
 * Launches: ONE.  The whole assignment of a structure stays in LDS -- N CA C O H of every residue, hb and its transpose as
 *   bits, the per-residue flags; nothing [S,R,R] reaches memory but hb_bits.  n_residues <= cgv_dssp_wave_path_max(): a wave
 *   owns a structure, four a block, the blocks walk the structures and gather class_counts in LDS.  Beyond: a block owns a
 *   structure.  Either way a lane owns a donor and the wave's ballot of the test is the word of hb; bridges and ladders are
 *   ANDs of shifted words.  Integer sums meet in atomicAdd: the same bits on every call, however the structures are cut.
 * No workspace.
 * Limits: 1 <= n_residues <= cgv_dssp_max_residues() -- 384: what 64 KB of LDS hold of 16 R W + 8 W + 67 R + 64 bytes -- and
 *   n_structures <= cgv_dssp_max_structures() per launch; beyond a limit the call fails (CGV_E_BADARG) with its reason before
 *   any launch.  See DESIGN.md (K26 row). */
int cgv_dssp_max_residues(void);
int cgv_dssp_max_structures(void);
int cgv_dssp_wave_path_max(void);
float cgv_dssp_bend_c2(void);
int cgv_dssp_assign(const float* xyz, const int32_t* res /*[R,4]*/, const int32_t* prev /*[R,2]*/, const int32_t* link /*[R]*/,
                    int n_structures, int n_atoms, int n_residues, int64_t* class_counts /*[R,8]*/, int32_t* n_class /*[S,8]*/,
                    int32_t* bad /*[S]*/, uint8_t* codes /*[S,R] or NULL*/, uint64_t* hb_bits /*[S,R,W] or NULL*/, void* stream);

/* ---------------------------------------------------------------------------------------
 * K27  Cartesian principal component analysis of a superposed ensemble ("essential dynamics", Amadei et al. 1993; what
 * gmx covar / gmx anaeig do) -- in which directions the atoms move TOGETHER.  Nothing in the reference computes it.
 * Both entry points read what K21 writes for a chunk of structures and never superpose anything themselves:
 *   y [n_structures,n_atoms,3] fp32           K21's `aligned`: the structures superposed onto a target
 *   bad [n_structures] int32                  K21's `bad`: a structure with bad[s] != 0 contributes nothing (its y is NaN
 *                                             and is never multiplied: all its features are staged as +0.0)
 *   sel [m] int32                             the atoms analysed, d = 3 m features.  An index outside [0, n_atoms) reads
 *                                             atom 0 (the host wrapper refuses such tables); nothing is read out of bounds.
 *   centre [n_atoms,3] fp64                   the point the sums are taken about: the caller passes the superposition
 *                                             target in the frame of y (its selected atoms' centroid at the origin), which
 *                                             is close to the mean, so nothing cancels when the covariance is formed
 * Feature:  f[3a + c] = (double)y[s, sel[a], c] - centre[sel[a], c],  a < m, c < 3.  The widening is exact and the
 * subtraction one fp64 rounding (no FMA contraction), so a host restatement holds the same bits.  No [n_structures, d]
 * feature tensor exists in memory.
 *
 * cgv_pca_moments ADDS, over the good structures, to the caller's buffers (zeroed by the caller before the first call)
 *   sum [d] fp64 += sum f      cov [d,d] fp64 += sum f f^T (full, exactly symmetric)      n_good [1] int32 += their number
 * Two launches: grid (tile pairs bi <= bj of 32 features, cgv_pca_moments_splits() structure ranges) x 256 threads, a
 * block stages 16 structures of its tiles' features in LDS as fp64 and accumulates F_i^T F_j in registers with
 * v_mfma_f64_16x16x4_f64 (the product is not rounded), diagonal blocks also sum their features in ascending structure
 * order; every block writes its tile to its range's slice of the workspace; the second launch sums the ranges in
 * ascending order into the totals and fills cov below the diagonal from above it.  No floating-point atomics: the order of
 * every addition is a function of (n_structures, d) alone -- the same bits on every run.  The ranges aim at about four
 * blocks per CU (K16's rule).
 * workspace: cgv_pca_moments_workspace_bytes(n_structures, d) bytes, 8-byte aligned, contents need not survive.
 *
 * cgv_pca_project: the structures onto k modes, mean [d] and W [d,k] fp64, 1 <= k <= cgv_pca_max_components() (8).  One
 * launch, one wave per structure.
 *   proj [n_structures,k] fp64 (may be NULL)  OVERWRITTEN: proj[s,c] = sum_f (f_s[f] - mean[f]) * W[f,c] (mean is passed,
 *                         not folded into an offset: two roundings per feature, restated bit for bit); each lane sums
 *                         features lane, lane + 64, .. in ascending order, a fixed xor tree combines the lanes (same bits
 *                         every run).  NaN for a bad structure.
 *   counts [n_bins2,n_bins2] int32, outside [1] int32 (both or neither; ZEROED BY THE CALLER, the launch ADDS)
 *                         the joint histogram of components (comp_a, comp_b), K16's bin rule: bin = floor((v - lo) *
 *                         n_bins2 / (hi - lo)) in fp64 for lo <= v < hi, clamped to [0, n_bins2); counts[bin_a, bin_b]; a
 *                         structure with either component outside its range or non-finite, and every bad structure,
 *                         counts once in outside.  LDS integer atomics, one integer vector atomic per non-zero slot.
 * Limits, each refused (CGV_E_BADARG) with its reason before any launch:
 *   3 m <= cgv_pca_max_features() -- 2048: bounded by total plus workspace bytes, a [d,d] fp64 total is 32 MB there and the
 *   workspace of a launch as much again (below 1409 features the ranges' slices together stay under 34 MB); m = 512 fits --
 *   n_atoms <= cgv_pca_max_atoms(), n_structures <= cgv_pca_max_structures() per launch, k <= cgv_pca_max_components(),
 *   1 <= n_bins2 <= cgv_pca_max_bins2(), lo < hi finite.  Bound: see DESIGN.md (K27 row). */
int cgv_pca_max_features(void);
int cgv_pca_max_atoms(void);
int cgv_pca_max_structures(void);
int cgv_pca_max_components(void);
int cgv_pca_max_bins2(void);
int cgv_pca_moments_splits(int n_structures, int d);                 /* structure ranges of a call; 0: the call adds nothing */
size_t cgv_pca_moments_workspace_bytes(int n_structures, int d);
int cgv_pca_moments(const float* y, const int32_t* sel /*[m]*/, const double* centre /*[n_atoms,3]*/, const int32_t* bad,
                    int n_structures, int n_atoms, int m, double* sum /*[3m]*/, double* cov /*[3m,3m]*/, int32_t* n_good,
                    void* workspace, size_t workspace_bytes, void* stream);
int cgv_pca_project(const float* y, const int32_t* sel /*[m]*/, const double* centre /*[n_atoms,3]*/, const int32_t* bad,
                    const double* mean /*[3m]*/, const double* W /*[3m,k]*/, int n_structures, int n_atoms, int m, int k,
                    double* proj /*[n_structures,k]*/, int comp_a, int comp_b, int n_bins2, double lo_a, double hi_a, double lo_b,
                    double hi_b, int32_t* counts, int32_t* outside, void* stream);

/* ---------------------------------------------------------------------------------------
 * K28  local distance difference test (lDDT, Mariani et al. 2013) and steric clashes of an ensemble -- how well every model
 * structure keeps the local distances of the reference structure it is scored against, WITHOUT superposition, per structure
 * and per atom, and how many pairs of non-bonded atoms overlap.  Nothing in the reference computes it.  Lengths in Angstrom.
 *   xyz [n_structures,n_atoms,3] fp32         the model structures
 *   ref_xyz [n_references,n_atoms,3] fp32     the reference structures
 *   ref_index [n_structures] int32, HOST      the reference of every model structure, in [0, n_references): checked here,
 *                                             then copied to the workspace on `stream` (the only host array of this header's
 *                                             analysis entry points; the caller renumbers it per launch anyway)
 *   sel [m] int32                             the selected atoms.  An index outside [0, n_atoms) reads atom 0 (the host
 *                                             wrapper refuses such tables); nothing is read out of bounds.
 *   excl_lddt, excl_clash [m,W] uint32, W = ceil(m / 32): bit (j & 31) of word j >> 5 of row i: the pair (i, j) never counts
 *                                             for the distance test / as a clash.  SYMMETRIC (the caller's duty: the
 *                                             per-atom counts walk ordered pairs); the diagonal never counts whatever the
 *                                             masks say; bits past m are ignored.
 *   radii [m] fp32                            of the selected atoms, for the clash test
 * For an unordered pair {i, j}, i != j, in fp32 with every operation individually rounded (no fma; sqrtf correctly rounded):
 *   q0 = sq_dist2(ref_i, ref_j), q = sq_dist2(x_i, x_j)      ((dx*dx + dy*dy) + dz*dz, csrc/sq_dist.h)
 *   included     iff  not excl_lddt  and  q0 < radius2       radius2: the CALLER's fp32(R0) * fp32(R0)
 *   e = fabsf(sqrtf(q) - sqrtf(q0))                          one rounded subtraction
 *   preserved_k  iff  included  and  e < t_k                 k = 0 .. 3, t0 < t1 < t2 < t3
 *   c = (r_i + r_j) - tolerance
 *   clash        iff  not excl_clash  and  c > 0  and  q < c * c
 * Every comparison is strict and false for a NaN.  A host that restates the arithmetic gets every integer below exactly; no
 * floating-point result leaves the device.  The six quantities, in this order: included, preserved_0 .. preserved_3, clash.
 *   struct_counts [n_structures,6] int32      overwritten: the six quantities of a structure over its pairs i < j
 *   atom_counts [m,6] int64                   ADDED to: the six quantities of selected atom i over the pairs {i, j} that
 *                                             contain it, summed over the good structures of this call; a caller cuts a long
 *                                             ensemble into launches and zeroes it once.  Over good structures
 *                                             sum_i atom_counts[i] = 2 sum_s struct_counts[s].
 *   bad [n_structures] int32                  overwritten: 1 for a structure with a non-finite coordinate in a selected
 *                                             atom, and for one whose reference has one.  Its struct_counts are -1, it
 *                                             enters no sum.  Atoms outside the selection are not looked at.
 * Launches: one wave per structure gathers the selection into a packed float4 copy in the workspace, first of the references
 *   (with a flag per reference), then of the models (bad, struct_counts = 0 or -1); then grid (column tiles of
 *   cgv_lddt_col_tile(), row tiles of cgv_lddt_row_tile(), slices of the structure axis) x 256 threads over the full grid of
 *   ordered pairs: a lane owns a row and the 32 columns of its wave, the row's six counters stay in registers;
 *   cgv_lddt_chunk() structures at a time go through LDS; sqrtf(q0) and the inclusion word of a thread's pairs stay in
 *   registers while ref_index does not change between consecutive good structures.  Per-structure counts take the pairs
 *   above the diagonal.  Integer sums meet in atomicAdd: the same bits on every call, however the structures are cut.
 * workspace: cgv_lddt_workspace_bytes(n_structures, n_references, m) bytes (0 beyond a limit), 16-byte aligned, contents
 *   need not survive.
 * Limits: 1 <= m <= cgv_lddt_max_atoms(), n_structures <= cgv_lddt_max_structures() and n_references <=
 *   cgv_lddt_max_references() per launch.  Beyond a limit, for a ref_index outside [0, n_references), for a radius2,
 *   threshold or tolerance that is not a finite number >= 0 and for thresholds that are not ascending the call fails
 *   (CGV_E_BADARG) with its reason before any launch; n_structures = 0 returns 0 and does nothing.  See DESIGN.md (K28 row). */
int cgv_lddt_max_atoms(void);
int cgv_lddt_max_structures(void);
int cgv_lddt_max_references(void);
int cgv_lddt_row_tile(void);
int cgv_lddt_col_tile(void);
int cgv_lddt_chunk(void);
size_t cgv_lddt_workspace_bytes(int n_structures, int n_references, int m);
int cgv_lddt_counts(const float* xyz, const float* ref_xyz, const int32_t* ref_index /*[S], host*/, const int32_t* sel /*[m]*/,
                    const uint32_t* excl_lddt /*[m,W]*/, const uint32_t* excl_clash /*[m,W]*/, const float* radii /*[m]*/,
                    int n_structures, int n_references, int n_atoms, int m, float radius2, float t0, float t1, float t2, float t3,
                    float tolerance, int32_t* struct_counts /*[S,6]*/, int64_t* atom_counts /*[m,6]*/, int32_t* bad /*[S]*/,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * K29  pair-distance distributions of an ensemble -- over the structures of a call, the histogram of the distances between
 * the pairs of selected atoms, one histogram per unordered pair of atom classes: the radial / pair distribution P(r).
 * Nothing in the reference computes it.  Lengths in Angstrom.
 *   xyz [n_structures,n_atoms,3] fp32         the structures
 *   sel [m] int32                             the selected atoms.  An index outside [0, n_atoms) reads atom 0 (the host
 *                                             wrapper refuses such tables); nothing is read out of bounds.
 *   cls [m] int32                             the class of every selected atom, in [0, n_classes); a value outside counts as
 *                                             class 0 (the host wrapper refuses such tables).  The unordered class pair
 *                                             (a <= b) has the index a * C - a * (a - 1) / 2 + (b - a), C = n_classes:
 *                                             P = C (C + 1) / 2 of them.
 *   excluded [m,W] uint32, W = ceil(m / 32)   bit (j & 31) of word j >> 5 of row i: the pair (i, j) never counts.  Only the
 *                                             bits j > i are read; the diagonal never counts; bits past m are ignored.
 * For a pair i < j that is not excluded, in fp32 with every operation individually rounded (no fma; sqrtf correctly rounded):
 *   q = sq_dist2(x_i, x_j)                    ((dx*dx + dy*dy) + dz*dz, csrc/sq_dist.h)
 *   in range  iff  q < rmax2                  strict, false for a NaN; rmax2: the CALLER's fp32(r_max) * fp32(r_max)
 *   b = min((int)(sqrtf(q) * scale), n_bins - 1)        scale: the CALLER's fp32(n_bins / fp32(r_max)), the quotient in fp64
 * A host that restates the arithmetic gets every integer below exactly; no floating-point result leaves the device.
 *   hist [P,n_bins] int64                     ADDED to: the in-range pairs of the good structures of this call, by class pair
 *                                             and bin; a caller cuts a long ensemble into launches and zeroes it once
 *   beyond [P] int64                          ADDED to: the pairs with q >= rmax2, by class pair.  For every class pair
 *                                             sum_b hist[p][b] + beyond[p] = good structures x its non-excluded pairs i < j.
 *   bad [n_structures] int32                  overwritten: 1 for a structure with a non-finite coordinate in a selected
 *                                             atom; it enters no sum.  Atoms outside the selection are not looked at.
 * Launches: one wave per structure gathers the selection into a packed float4 copy in the workspace and decides bad; then
 *   grid (column tiles of cgv_pairdist_col_tile(), row tiles of cgv_pairdist_row_tile(), slices of the structure axis) x 256
 *   threads over the tiles that hold a pair i < j: a lane owns a row and the 32 columns of its wave; cgv_pairdist_chunk()
 *   structures at a time go through LDS; the block's histogram is private in LDS (32-bit counters, integer LDS atomics; as
 *   many as four copies, chosen by lane, where they fit 64 KB with the staging; the pairs beyond r_max are counted in
 *   registers first) and is added to hist / beyond once, one 64-bit atomicAdd per nonzero counter.  A block counts at most 2^13 pairs x 2^18 structures = 2^31: no 32-bit counter wraps.  Integer sums meet
 *   in atomicAdd: the same bits on every call, however the structures are cut.
 * workspace: cgv_pairdist_workspace_bytes(n_structures, m) bytes (0 beyond a limit), 16-byte aligned, contents need not
 *   survive.
 * Limits: 1 <= m <= cgv_pairdist_max_atoms(), n_structures <= cgv_pairdist_max_structures() per launch, 1 <= n_classes <=
 *   cgv_pairdist_max_classes(), 1 <= n_bins <= cgv_pairdist_max_bins().  Beyond a limit, for an rmax2 that is not a finite
 *   number >= 0 and for a scale that is not a finite number > 0 the call fails (CGV_E_BADARG) with its reason before any
 *   launch and writes nothing; n_structures = 0 returns 0 and does nothing.  See DESIGN.md (PD row). */
int cgv_pairdist_max_atoms(void);
int cgv_pairdist_max_structures(void);
int cgv_pairdist_max_classes(void);
int cgv_pairdist_max_bins(void);
int cgv_pairdist_row_tile(void);
int cgv_pairdist_col_tile(void);
int cgv_pairdist_chunk(void);
size_t cgv_pairdist_workspace_bytes(int n_structures, int m);
int cgv_pairdist_counts(const float* xyz, const int32_t* sel /*[m]*/, const int32_t* cls /*[m]*/, const uint32_t* excluded /*[m,W]*/,
                        int n_structures, int n_atoms, int m, int n_classes, int n_bins, float rmax2, float scale,
                        int64_t* hist /*[P,n_bins]*/, int64_t* beyond /*[P]*/, int32_t* bad /*[S]*/, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * K30  distance-matrix moments of an ensemble -- over the structures of a call, for every pair of selected atoms the sum and
 * the sum of squares of its distance minus a centre (the mean-distance map, the standard-deviation map, ens_dRMS), and per
 * structure the sum of the squared deviations of its distances from the centre table (the superposition-free distance RMSD
 * to a target map).  Nothing in the reference computes it.  Lengths in Angstrom.
 *   xyz [n_structures,n_atoms,3] fp32         the structures
 *   sel [m] int32                             the selected atoms.  An index outside [0, n_atoms) reads atom 0 (the host
 *                                             wrapper refuses such tables); nothing is read out of bounds.
 *   excluded [m,W] uint32, W = ceil(m / 32)   or NULL (no pair is left out).  Bit (j & 31) of word j >> 5 of row i: the pair
 *                                             (i, j) enters no sum.  Only the bits j > i are read; the diagonal never
 *                                             counts; bits past m are ignored.
 *   center [m,m] fp32                         or NULL (zeros).  Symmetric; only the entries j > i of the pairs that count
 *                                             are read.  An entry outside [0, 1024] or a NaN is read as 0 (the host wrapper
 *                                             refuses such tables).
 * For a good structure s and a pair i < j that is not excluded, in fp32 with every operation individually rounded (no fma;
 * sqrtf correctly rounded):
 *   q = sq_dist2(x_i, x_j)   d = sqrtf(q)   e = d - center[i][j]   f = e * e            (csrc/sq_dist.h)
 *   sum_e[i][j] += rint(e * 2^20)     sum_e2[i][j] += rint(f * 2^20)     dev2[s] += rint(f * 2^12)
 * The products by a power of two are exact and rint is ties-to-even: a host that restates the arithmetic gets every integer
 * below exactly; no floating-point result leaves the device.
 *   sum_e, sum_e2 [m,m] int64                 ADDED to, at [i][j] and [j][i]: a caller cuts a long ensemble into launches and
 *                                             zeroes them once; the diagonal and the excluded pairs are never written
 *   dev2 [n_structures] int64                 ADDED to: the caller zeroes it; a bad structure's stays as it was
 *   bad [n_structures] int32                  overwritten: 1 for a structure with a non-finite coordinate in a selected atom
 *                                             or a selected atom more than 512 A from the centroid of the selection (fp64);
 *                                             it enters no sum.  Atoms outside the selection are not looked at.
 * Launches: one wave per structure gathers the selection into a packed float4 copy in the workspace and decides bad; then
 *   grid (column tiles of cgv_dist_moments_col_tile(), row tiles of cgv_dist_moments_row_tile(), slices of the structure
 *   axis) x 256 threads over the tiles that hold a pair i < j: a lane owns a row and 16 columns with their centres and int64
 *   sums in registers; cgv_dist_moments_chunk() structures at a time go through LDS; dev2 goes through int64 LDS counters of
 *   the chunk.  Integer sums meet in atomicAdd: the same bits on every call, however the structures are cut.
 * Overflow: |e| <= 2^10 and f <= 2^20 (the 512 A rule and the centre's range), so with at most cgv_dist_moments_max_total()
 *   = 2^22 good structures accumulated into one pair of tables |sum_e| <= 2^52 and sum_e2 <= 2^62 (each times 1 + 2^-20 for
 *   the rounding of d), and dev2 < 2^25 pairs x 2^32.  The CALLER keeps the total; the host wrapper refuses more.
 * workspace: cgv_dist_moments_workspace_bytes(n_structures, m) bytes (0 beyond a limit), 16-byte aligned, contents need not
 *   survive.
 * Limits: 2 <= m <= cgv_dist_moments_max_atoms(), n_structures <= cgv_dist_moments_max_structures() per launch.  Beyond a
 *   limit the call fails (CGV_E_BADARG) with its reason before any launch and writes nothing; n_structures = 0 returns 0
 *   and does nothing.  See DESIGN.md (DM row). */
int cgv_dist_moments_max_atoms(void);
int cgv_dist_moments_max_structures(void);
int cgv_dist_moments_max_total(void);
int cgv_dist_moments_row_tile(void);
int cgv_dist_moments_col_tile(void);
int cgv_dist_moments_chunk(void);
size_t cgv_dist_moments_workspace_bytes(int n_structures, int m);
int cgv_dist_moments(const float* xyz, const int32_t* sel /*[m]*/, const uint32_t* excluded /*[m,W] or NULL*/,
                     const float* center /*[m,m] or NULL*/, int n_structures, int n_atoms, int m, int64_t* sum_e /*[m,m]*/,
                     int64_t* sum_e2 /*[m,m]*/, int64_t* dev2 /*[S]*/, int32_t* bad /*[S]*/, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * K31  stereochemistry of an ensemble -- over the structures of a call, how often every stereocentre is of the negative hand
 * or flat, how often every torsion about a bond that does not rotate is cis, how often every bond pierces every ring, and
 * per structure the centres of the wrong hand, the torsions in the wrong state and the pierced (ring, bond) pairs.  Nothing
 * in the reference computes it.
 *   xyz [n_structures,n_atoms,3] fp32         the structures
 *   sel [P] int32                             the atoms that the tables name.  An index outside [0, n_atoms) reads atom 0.
 *   centres [C,4], torsions [Q,4] int32       (c, a, b, d) and (i, j, k, l): PLACES in sel
 *   rings [R, cgv_stereo_max_ring()] int32    places in sel along the cycle, 3 to 8 of them, then -1; a row with fewer than
 *                                             3 is pierced by nothing
 *   bonds [B,2] int32                         places in sel
 *                                             A place outside [0, P) reads place 0 (the host wrapper refuses such tables);
 *                                             nothing is read out of bounds.
 *   tested [R,W] uint32, W = ceil(B / 32)     bit (b & 31) of word b >> 5 of row r: the pair (ring r, bond b) is looked at;
 *                                             bits past B are ignored
 *   want_sign [C] int32 (-1 / +1), want_cis [Q] int32 (0 / 1)      or NULL: that counter of `counts` stays 0
 * In fp32 with every operation individually rounded (no fma, no square root, no division), with
 *   x(u, v) = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x)      d(u, v) = (u.x*v.x + u.y*v.y) + u.z*v.z
 *   centre   V = d(a - c, x(b - c, d - c))                     negative: V < 0      flat: V == 0
 *   torsion  X = d(x(j - i, k - j), x(k - j, l - k))           cis: X > 0
 *   ring v_0 .. v_{k-1} against the bond (p0, p1):   g = (((v_0 + v_1) + v_2) + ...) * fp32(1 / k),  dir = p1 - p0,  tvec = p0 - g;
 *     for every triangle (g, v_t, v_{t+1 mod k}) of the fan:  e1 = v_t - g, e2 = v_{t+1} - g,
 *       pv = x(dir, e2)   det = d(e1, pv)   u' = d(tvec, pv)   q = x(tvec, e1)   v' = d(dir, q)   t' = d(e2, q)   w' = u' + v'
 *       crossed:  det > 0 and u' >= 0 and v' >= 0 and w' <= det and t' >= 0 and t' <= det
 *             or  det < 0 and u' <= 0 and v' <= 0 and w' >= det and t' <= 0 and t' >= det         (det == 0: not crossed)
 *     pierced: at least one triangle is crossed.  There is no pre-filter: every tested pair gets the full fan.
 * A host that restates the arithmetic gets every integer below exactly; no floating-point result leaves the device.
 *   neg, flat [C] int64, cis [Q] int64        ADDED to: the good structures in which the centre is negative / flat, the
 *                                             torsion cis.  The caller zeroes them once and may cut an ensemble into launches.
 *   pierced [R,B] int32                       ADDED to, and only where a tested pair is pierced
 *   counts [n_structures,3] int32             overwritten: centres whose sign (-1, 0 for flat, +1) differs from want_sign,
 *                                             torsions whose state differs from want_cis, pierced tested pairs; 0 for a bad
 *                                             structure
 *   bad [n_structures] int32                  overwritten: 1 for a structure with a non-finite coordinate among the atoms of
 *                                             sel; it enters nothing.  Atoms outside sel are not looked at.
 * Launches: one wave per structure gathers sel, and the R ring centres, into a packed float4 copy in the workspace; a light
 *   pass with a lane per centre or torsion (tiles of cgv_stereo_item_tile()); then grid (tiles of cgv_stereo_col_tile()
 *   bonds, tiles of cgv_stereo_row_tile() rings, slices of the structure axis) x 256 threads with cgv_stereo_chunk()
 *   structures at a time in LDS.  Integer sums meet in atomicAdd: the same bits on every call, however the structures are cut.
 *   C, Q, R, B may each be 0; with all four 0 only bad (and counts = 0) is written.
 * workspace: cgv_stereo_workspace_bytes(n_structures, P, R) bytes (0 beyond a limit), 16-byte aligned, contents need not
 *   survive.
 * Limits: cgv_stereo_max_structures() per launch, P <= cgv_stereo_max_atoms() and <= n_atoms, cgv_stereo_max_centres(),
 *   _torsions(), _rings(), _bonds().  Beyond a limit the call fails (CGV_E_BADARG) with its reason before any launch and
 *   writes nothing; n_structures = 0 returns 0 and does nothing.  See DESIGN.md (ST row). */
int cgv_stereo_max_structures(void);
int cgv_stereo_max_atoms(void);
int cgv_stereo_max_centres(void);
int cgv_stereo_max_torsions(void);
int cgv_stereo_max_rings(void);
int cgv_stereo_max_bonds(void);
int cgv_stereo_max_ring(void);
int cgv_stereo_item_tile(void);
int cgv_stereo_row_tile(void);
int cgv_stereo_col_tile(void);
int cgv_stereo_chunk(void);
size_t cgv_stereo_workspace_bytes(int n_structures, int n_sel, int n_rings);
int cgv_stereo_counts(const float* xyz, const int32_t* sel /*[P]*/, const int32_t* centres /*[C,4]*/, const int32_t* torsions /*[Q,4]*/,
                      const int32_t* rings /*[R,8]*/, const int32_t* bonds /*[B,2]*/, const uint32_t* tested /*[R,W]*/,
                      const int32_t* want_sign /*[C] or NULL*/, const int32_t* want_cis /*[Q] or NULL*/, int n_structures,
                      int n_atoms, int n_sel, int n_centres, int n_torsions, int n_rings, int n_bonds, int64_t* neg /*[C]*/,
                      int64_t* flat /*[C]*/, int64_t* cis /*[Q]*/, int32_t* pierced /*[R,B]*/, int32_t* counts /*[S,3]*/,
                      int32_t* bad /*[S]*/, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * K32  restrained geometry relaxation of an ensemble -- `steps` damped Jacobi steps of every structure towards the restraint
 * table's distances and out of its steric clashes (K28's predicate), a weak spring holding every atom at its anchor.  The
 * one entry point that returns coordinates.  Nothing in the reference computes it.
 *   xyz, anchor [n_structures,n_atoms,3] fp32   the structures and where their atoms are held (may be the same pointer)
 *   row_ptr [n_atoms+1], partner, d0, w [E]     the restraints in per-atom CSR form: every restraint {i, j} under both atoms,
 *                                               an atom's entries in the order of the host table.  A partner outside
 *                                               [0, n_atoms) reads atom 0 and a row_ptr outside [0, E] is clamped (the host
 *                                               wrapper refuses such tables); nothing is read out of bounds.
 *   wsum [n_atoms] fp32                         W_i: the fp32 sum of the atom's w in table order, made on the host
 *   radii [n_atoms] fp32, excl [n_atoms,W] uint32, W = ceil(n_atoms / 32)      bit (j & 31) of word j >> 5 of row i: the pair is
 *                                               no clash whatever its distance (ensemble.pack_mask)
 * In fp32 with every operation individually rounded (sqrtf and / correctly rounded), for atom i from the positions of the
 * PREVIOUS step (two buffers, a barrier between steps: nothing depends on which thread owns which atom):
 *   g = k_pos * (x_i - a_i)
 *   restraints in table order:   D = x_i - x_j, q = (D.x*D.x + D.y*D.y) + D.z*D.z; if q > 0: d = sqrtf(q), g = g + ((w * (d - d0)) / d) * D
 *   j ascending, j != i, not excl:   c = (r_i + r_j) - tol; if c > 0 and q < c * c and q > 0: g = g + ((k_rep * (d - c)) / d) * D, nc += 1
 *   h = (k_pos + 2 * W_i) + (2 * k_rep) * float(nc)
 *   h > 0:  delta = (-(damp / h)) * g;  m = (delta.x^2 + delta.y^2) + delta.z^2;  if m > cap * cap: delta = delta * (cap / sqrtf(m))
 *   x_i' = x_i + delta                                                          (h > 0 fails: delta = 0)
 * A host that restates the arithmetic gets xyz_out, clashes, disp2 and bad bit for bit.
 *   xyz_out [n_structures,n_atoms,3] fp32       overwritten; must not overlap xyz or anchor
 *   clashes [n_structures,2] int32              the pairs i < j with c > 0 and q < c * c before the first step and after the last
 *   energy [n_structures,2] fp64                before and after: per atom, in fp64 from the fp32 distances,
 *                                               (0.5 k_pos) |x - a|^2, (0.25 w)(d - d0)^2 per entry, (0.25 k_rep)(d - c)^2 per
 *                                               clashing partner, summed in a fixed tree (no floating-point atomics): the same
 *                                               bits on every call, within N_terms * 2^-53 relative of the exact sum
 *   disp2 [n_structures] fp32                   the largest squared displacement from the anchor after the last step
 *   bad [n_structures] int32                    1 for a structure with a non-finite coordinate or anchor: its coordinates are
 *                                               copied through and its other outputs are 0
 * steps = 0 copies the input and reports the same before and after.
 * Launch: 256 threads; cgv_relax_pack(n_atoms) structures share a block (4 for up to 64 atoms, 2 for up to 128, else 1), each
 *   resident in LDS (44 bytes an atom) for all steps; a thread owns the atoms t, t + T, ...
 * Limits: cgv_relax_max_structures() per launch, n_atoms <= cgv_relax_max_atoms() (what fits a CU's 160 KB of LDS),
 *   steps <= cgv_relax_max_steps(); k_pos, k_rep, tol, damp finite and >= 0, cap finite and > 0.  Beyond a limit the call fails
 *   (CGV_E_BADARG) with its reason before any launch and writes nothing; n_structures = 0 returns 0 and does nothing. */
int cgv_relax_max_atoms(void);
int cgv_relax_max_structures(void);
int cgv_relax_max_steps(void);
int cgv_relax_pack(int n_atoms);
int cgv_relax(const float* xyz, const float* anchor, const int32_t* row_ptr /*[n+1]*/, const int32_t* partner /*[E]*/,
              const float* d0 /*[E]*/, const float* w /*[E]*/, const float* wsum /*[n]*/, const float* radii /*[n]*/,
              const uint32_t* excl /*[n,W]*/, int n_structures, int n_atoms, int n_entries, float k_pos, float k_rep, float tol,
              float damp, float cap, int steps, float* xyz_out, int32_t* clashes /*[S,2]*/, double* energy /*[S,2]*/,
              float* disp2 /*[S]*/, int32_t* bad /*[S]*/, void* stream);

/* ---------------------------------------------------------------------------------------
 * K33  weighted pair-distance histograms of an ensemble, one per structure: what the small-angle scattering profile I(q),
 * the weighted P(r), Rg and Dmax of every structure are made from on the host (saxs.py).  Nothing in the reference computes
 * it.
 *   xyz [n_structures,n_atoms,3] fp32, sel [m]  the structures and the selected atoms (an index outside [0, n_atoms) reads
 *                                               atom 0; the host wrapper refuses such a table)
 *   wq [m] int32                                the fixed-point weight of every selected atom, |wq| <= cgv_saxs_max_weight()
 *                                               (the host's rint(w * 16); the kernel multiplies whatever it is given in 32 bits)
 * For a good structure s and EVERY pair i < j of the selection (no exclusion mask), in fp32 with every operation
 * individually rounded (sqrtf correctly rounded) -- K29's bin rule:
 *   q = (dx*dx + dy*dy) + dz*dz;  in range iff q < rmax2 (strict);  b = min((int)(sqrtf(q) * scale), n_bins - 1)
 *   in range:  hist[s][b] += wq_i * wq_j          otherwise:  beyond[s] += 1   (a count of pairs, whatever their weights)
 *   hist [n_structures,n_bins] int64, beyond [n_structures] int64      ADDED to: the caller zeroes them; integer atomics only
 *   bad [n_structures] int32                    overwritten: 1 for a structure with a non-finite selected coordinate, which
 *                                               adds nothing to its rows
 * A host that restates the arithmetic gets every integer; no floating-point number leaves the device; the same bits on
 * every call, however the structures are cut into launches and however many blocks share a structure.
 *   split                                       0: the library decides how many blocks share a structure of more than
 *                                               cgv_saxs_small() atoms (cgv_saxs_blocks); > 0: that many, at most one per
 *                                               row tile -- for tests and measurements, the result does not depend on it
 * Launch: a preparation launch (one wave per structure) packs the selection into the workspace; then, for m <=
 *   cgv_saxs_small(), cgv_saxs_pack(m, n_bins) structures share a block, a wave each; else cgv_saxs_blocks() blocks of 256
 *   threads share a structure, each walking its row tiles (cgv_saxs_row_tile() x cgv_saxs_col_tile()) above the diagonal.
 *   The block's histogram is private in LDS, n_bins signed 64-bit cells.
 * Overflow: |wq_i wq_j| < 2^30, fewer than 2^25 pairs per structure: |hist[s][b]| < 2^55.
 * Limits: cgv_saxs_max_structures() per launch, m <= cgv_saxs_max_atoms(), n_bins <= cgv_saxs_max_bins(); rmax2 finite and
 *   >= 0, scale finite and > 0.  Beyond a limit the call fails (CGV_E_BADARG) with its reason before any launch and writes
 *   nothing; n_structures = 0 returns 0 and does nothing.  workspace: cgv_saxs_workspace_bytes() bytes (0 for sizes beyond
 *   the limits), 16-byte aligned. */
int cgv_saxs_max_atoms(void);
int cgv_saxs_max_structures(void);
int cgv_saxs_max_bins(void);
int cgv_saxs_max_weight(void);
int cgv_saxs_row_tile(void);
int cgv_saxs_col_tile(void);
int cgv_saxs_small(void);
int cgv_saxs_pack(int m, int n_bins);
int cgv_saxs_blocks(int n_structures, int m, int split);
size_t cgv_saxs_workspace_bytes(int n_structures, int m);
int cgv_saxs_hist(const float* xyz, const int32_t* sel /*[m]*/, const int32_t* wq /*[m]*/, int n_structures, int n_atoms, int m,
                  int n_bins, float rmax2, float scale, int split, int64_t* hist /*[S,n_bins]*/, int64_t* beyond /*[S]*/,
                  int32_t* bad /*[S]*/, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CGVAE_HIP_H */
