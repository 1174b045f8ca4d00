/*
 * fgc.h - C ABI of libfgc.so, the MI355X (gfx950) facet-graph-convolution kernels.
 *
 * The reference (Elensil/Facet_Graph_Convolution) has no FFI: its "operator API" is the
 * set of Python functions in Code/model.py that build TensorFlow graph nodes.  This
 * header is the boundary a maintainer would bind instead (ctypes stub: INTEGRATION.md);
 * each entry point names the reference symbol (file:line) it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _h (host);
 *   - the caller owns every buffer; the library allocates nothing and never synchronises;
 *   - kernels are enqueued on `stream` (a hipStream_t passed as void*); 0 = default stream;
 *   - return 0 on success, a negative FGC_E* code otherwise; fgc_last_error() gives the
 *     text for the calling thread;
 *   - float tensors are fp32 row-major with channels innermost ([n, C]); index tensors int32;
 *   - M (number of soft-assignment weight matrices) is fixed to FGC_M = 9 (model.py:855).
 *
 * Adjacency: the reference K-list (int32 [n, K], one-indexed, 0 = empty slot, slot 0 =
 * self; utils.py:243-295, utils.py:1799-1827) is converted once to CSR that PRESERVES
 * slot order and duplicates: col[rowptr[i] .. rowptr[i+1]) = adj[i, k] - 1 over the
 * non-zero slots k in increasing k.  deg(i) = rowptr[i+1] - rowptr[i] = count_nonzero
 * (model.py:436).
 */
#ifndef FGC_H
#define FGC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FGC_M 9            /* soft-assignment matrices per conv (model.py:855,868,880) */
#define FGC_AG_LD 24       /* row stride of the assignment-logit table: a[0..8] pad, g[12..20] pad */
#define FGC_DL_LD 12       /* row stride of the per-edge dlogit buffer */

#define FGC_OK 0
#define FGC_EINVAL (-22)
#define FGC_ENOMEM (-12)
#define FGC_EHIP (-5)

/* ABI version of this header.  fgc_version() returns the value the LIBRARY was built with: a binding compares the two
 * (and the struct sizes below) before its first call.  102: fgc_set_option / fgc_get_option; fgc_conv_pack(extra),
 * flags of fgc_mlp_fwd / fgc_mlp_bwd and their _bf16 forms, larger fgc_conv_desc / fgc_conv_bwd_io (all since 101).
 * 103: fgc_conv_pairs_allowed; options NO_BFM, K1_QS14; fgc_conv_desc.options / n_options (per-descriptor option overrides).
 * 104: fgc_conv_bwd_io.r_ld (the stride of r stated with the buffer); fgc_conv_desc.packed_layout + fgc_conv_layout_id,
 * fgc_mlp_layout_id / FGC_MLP_LAYOUT (packed operands carry the identity of their layout).
 * 105: fgc_nn_query / fgc_nn_workspace_bytes (nearest neighbour over point sets, for the evaluation metrics).
 * 106: fgc_vertex_update_ms_traj / fgc_vertex_update_ms_bwd (+ _workspace_floats), fgc_point_loss (+ _workspace_bytes):
 * training through the multi-scale vertex update on the point-set loss.
 * 107: fgc_dense_normals_loss_fwd / _bwd (+ _scratch_floats): the face-normal loss over all rows, for training on the
 * point-set and face-normal losses together.
 * 108: fgc_bilateral_filter / fgc_bilateral_workspace_bytes (bilateral normal filtering, the classical baseline).
 * 109: fgc_synth_noise / fgc_face_features_rows (+ fgc_synth_scratch_floats, fgc_philox_words): per-step noise synthesis on
 * a clean mesh.
 * 110: options K1_QS14 and W8_HALF2 removed with the two kernel forms they selected (both measured slower; the later option
 * indices do not move: the two were last in the table).
 * 111: fgc_conv_forms (which kernel form every launch of a layer takes, as text).
 * 112: fgc_point_sets_prepare (the two point sets of the point-set loss normalised together and rotated, on the device:
 * the vertex networks trained from clean meshes).
 * 113: fgc_mlp_forms (which kernel form a call of the MLP head takes, as text); fgc_mlp_fwd / fgc_mlp_bwd refuse a workspace
 * that is not 16-byte aligned (every kernel form reads its packed W1 in 16-byte pieces).
 * 114: fgc_synth_noise_lf (+ fgc_synth_lf_scratch_floats): low-frequency noise, a field of Gaussian bumps on top of the
 * per-vertex draw of fgc_synth_noise.
 * 115: fgc_guided_normals / fgc_guided_workspace_bytes / fgc_bilateral_filter_guided (guided normal filtering);
 * fgc_bilateral_workspace_bytes grows by one float4 per face, the guided form's third candidate plane (one size for both).
 * 116: fgc_vertex_update_dir (+ _workspace_floats): the vertex update along a per-vertex direction, for depth scans.
 * Added under 116, the number unchanged (new entry points only: nothing a 116 binding calls has moved, and a binding that
 * declares them finds out at load time whether the library has them): fgc_vertex_update_ms_dir / _traj / _bwd
 * (+ _scratch_floats, _bwd_workspace_floats), the multi-scale vertex update along a per-vertex direction and its adjoint,
 * depth scans for the vertex networks; fgc_ray_cast (+ _workspace_bytes), rays against a triangle list: virtual depth
 * scans of a clean mesh; fgc_ray_tree_bytes / fgc_ray_tree_build / fgc_ray_cast_tree, the same cast through a bounding-box
 * tree: scans of large meshes; fgc_synth_noise_sensor, the noise of a triangulating depth sensor along the viewing rays:
 * sigma grows with the range, depth is quantised in disparity; fgc_closest_point_tree, the closest point on a mesh through
 * the same tree: distances to a surface; fgc_closest_point (+ _workspace_bytes), the closest point without a tree, and
 * fgc_surface_loss (+ _workspace_bytes), the point-to-surface loss and its gradient: the vertex networks trained against a
 * ground-truth mesh of any topology. */
#define FGC_ABI_VERSION 116

const char* fgc_last_error(void);
int fgc_version(void);
/* Process-level options: which kernel form a launch takes where the library has more than one (A/B switches and
 * developer knobs; the defaults are the measured best).  Names are those of csrc/fgc_common.h's FGC_OPTION_LIST, with or
 * without an "FGC_" prefix ("NO_PAIRS", "FGC_W8_DATA16_MIN_N", ...).  The table is filled ONCE per process, the first time
 * any option is read, from environment variables FGC_<NAME>; after that only fgc_set_option changes it and no launch path
 * reads the environment.  Values apply to the calls that follow; do not change an option between a call that packs or
 * plans (fgc_conv_pack, the *_workspace_bytes queries, fgc_conv_uses_pairs) and the calls that consume its result.
 * fgc_option_name(i), 0 <= i < fgc_option_count(), enumerates the names.  Unknown name: FGC_EINVAL. */
int fgc_set_option(const char* name, int64_t value);
int fgc_get_option(const char* name, int64_t* value);
int32_t fgc_option_count(void);
const char* fgc_option_name(int32_t index);
/* sizeof the descriptor structs as this library was compiled (which = 0: fgc_conv_desc, 1: fgc_conv_bwd_io,
 * 2: fgc_pack_extra; else 0):
 * lets a foreign-language binding check its mirror of the layouts before the first call */
size_t fgc_struct_size(int32_t which);

/* Optional per-kernel timing (hipEvents around every launch of the library; off by default, not
 * capturable into a hipGraph while on).  fgc_profile_collect synchronises and writes one line
 * "tag/kernel count total_ms" per distinct kernel into buf; returns the bytes written. */
int fgc_profile_enable(int on);
int fgc_profile_tag(const char* tag);
int fgc_profile_collect(char* buf, int32_t buf_bytes);

/* ------------------------------------------------------------------------------------
 * Host-side graph conversion (CPU; pointers are HOST pointers)
 * ---------------------------------------------------------------------------------- */

/* K-list -> CSR.  rowptr_h [n+1]; col_h may be NULL to query nnz only.
 * replaces: the K-padded adjacency fed to get_slices/get_patches (model.py:380-405). */
int fgc_csr_from_klist(const int32_t* adj_h, int32_t n, int32_t K, int32_t* rowptr_h, int32_t* col_h,
                       int64_t* nnz_out);
/* CSR -> K-list (zero padded).  Bit-identical round trip for rows whose zeros are trailing. */
int fgc_klist_from_csr(const int32_t* rowptr_h, const int32_t* col_h, int32_t n, int32_t K, int32_t* adj_h);
/* Transposed CSR for the backward pass: for every node j the list of (i, e) such that forward
 * edge e = (i -> j); in-edges ordered by e.  trowptr_h [n+1], tcol_h [nnz] (= i), tedge_h [nnz] (= e). */
int fgc_csr_transpose(const int32_t* rowptr_h, const int32_t* col_h, int32_t n, int32_t* trowptr_h,
                      int32_t* tcol_h, int32_t* tedge_h);
/* Parent-compressed ("pair") graph of a level whose convolution reads a 4x-upsampled coarse tensor
 * (custom_upsampling model.py:817-825 feeding custom_conv2d at model.py:905,926; n % 4 == 0).  Neighbour j of a fine
 * node contributes the coarse row j >> 2, and the soft assignment of edge (i, j) (model.py:74-95) depends on
 * (i >> 2, j >> 2) only: all edges of the four siblings of block p = i >> 2 into one coarse row P are ONE pair (p, P)
 * with four multiplicities.  prow_h [n/4 + 1]; pcol_h [n_pairs] = P, ascending inside a block; pmul_h [n_pairs] =
 * multiplicity of P in the list of child 0 | child 1 << 8 | child 2 << 16 | child 3 << 24 (each < 256).
 * pcol_h = pmul_h = NULL: count only.  The transposed pair graph is fgc_csr_transpose(prow, pcol, n/4). */
int fgc_pair_graph(const int32_t* rowptr_h, const int32_t* col_h, int32_t n, int32_t* prow_h, int32_t* pcol_h,
                   uint32_t* pmul_h, int64_t* n_pairs_out);

/* ------------------------------------------------------------------------------------
 * Host-side mesh preprocessing (CPU, native C++; HOST pointers).  These replace the Python loops that
 * build the tensors the network is fed (dataClasses.py:34-233).
 * ---------------------------------------------------------------------------------- */

/* unit face normals (computeFacesNormals utils.py:63-68 + normalize utils.py:26-35, fp32) and face
 * barycentres divided by the bounding-box diagonal (getTrianglesBarycenter utils.py:1264-1294, fp32
 * arithmetic stored as double like the reference's float64 array).  V [nv,3] f32, F [nf,3] u32. */
int fgc_face_features(const float* V_h, int32_t nv, const uint32_t* F_h, int32_t nf, float* normals_h,
                      double* centres_h);
/* vertex-sharing facet adjacency K-list (getFacesLargeAdj utils.py:243-295), bit-exact: row i =
 * [i+1, neighbours+1 in construction order (edge neighbours twice), 0...].  *unregistered counts the
 * connections dropped because a row was full. */
int fgc_faces_large_adj(const uint32_t* F_h, int32_t nf, int32_t nv, int32_t K, int32_t* adj_h,
                        int64_t* unregistered);
/* one greedy pairing pass (metis_one_level lib/coarsening.py:135-192), bit-exact given its arguments */
int fgc_metis_one_level(const int32_t* rr_h, const int32_t* cc_h, const float* vv_h, int64_t nnz,
                        const int64_t* rid_h, const float* weights_h, int32_t N, int32_t* cluster_id_h,
                        double* total_assoc);
/* Graph hierarchy = listToSparseWNormals (utils.py:1753-1796) + coarsen (lib/coarsening.py:5-31).
 * The handle owns host memory (the only allocation the library makes); free it with fgc_hierarchy_free.
 * parents_h (optional): `levels` recorded cluster-assignment arrays to replay (then `seed` is unused and the
 * result is bit-identical to the reference run that produced them); parents_len_h their lengths. */
typedef struct fgc_hierarchy fgc_hierarchy;
int fgc_hierarchy_build(const int32_t* adj_h, int32_t n, int32_t K, const double* pos_h, const float* normals_h,
                        int32_t levels, uint64_t seed, const int32_t* const* parents_h,
                        const int32_t* parents_len_h, fgc_hierarchy** out);
void fgc_hierarchy_free(fgc_hierarchy* h);
int32_t fgc_hierarchy_size(const fgc_hierarchy* h, int32_t level);       /* padded node count */
int32_t fgc_hierarchy_real_size(const fgc_hierarchy* h, int32_t level);  /* before fake nodes */
int fgc_hierarchy_new_to_old(const fgc_hierarchy* h, int32_t level, int32_t* out_h);
int fgc_hierarchy_parents(const fgc_hierarchy* h, int32_t level, int32_t* out_h);
/* K-list of graph `level` in binary-tree order (perm_adjacency coarsening.py:269-296 + sparseToList
 * utils.py:1799-1827); *saturated = 1 if a row had more than K-1 neighbours. */
int fgc_hierarchy_klist(const fgc_hierarchy* h, int32_t level, int32_t K, int32_t* adj_h, int32_t* saturated);

/* Breadth-first patch of a facet graph = getGraphPatch_wMask (utils.py:1508-1696), host: what the reference cuts
 * meshes above MAX_PATCH_SIZE into (dataClasses.py:76-171).  adj_h [n, K] one-indexed K-list, mask_h [n] (1 = node
 * already covered by an earlier patch: added as context, expanded only while the patch is below min_patch_size).
 * Outputs: patch_adj_h [nodes_num + K, K] one-indexed K-list of the patch in discovery order (rows of expanded nodes
 * keep their slots, rows of nodes still queued when growth stopped are compacted), old_index_h [nodes_num + K],
 * *patch_n the number of nodes written, *next_seed an uncovered node seen just outside the patch or -1.
 * Same queue discipline as the reference, so all three are bit-identical to its output. */
int fgc_graph_patch(const int32_t* adj_h, int32_t n, int32_t K, int32_t nodes_num, int32_t seed, const int8_t* mask_h,
                    int32_t min_patch_size, int32_t* patch_adj_h, int32_t* old_index_h, int32_t* patch_n,
                    int32_t* next_seed);

/* Breadth-first patch of a MESH = getMeshPatch (utils.py:1298-1410), host: what the multi-scale pipeline cuts meshes
 * above maxSize into (dataClasses.py:270-372).  V_h [nv,3], F_h [nf,3] int32, adj_h [nf,K] one-indexed K-list of the
 * faces.  Grows from face `seed` until face_num faces are in (plus the at most K-1 discovered by the last expanded
 * face).  Outputs, all in discovery order: v_out_h [v_cap,3] vertices of the patch (v_cap = int(0.6 * face_num) + K in
 * the reference; -EINVAL where the reference raises IndexError), f_out_h [face_num+K,3] faces in patch vertex ids,
 * adj_out_h [face_num+K,K] their one-indexed K-list (rows of faces still queued when growth stopped are compacted),
 * v_old_h / f_old_h the mesh index of every patch vertex / face, *n_v / *n_f the counts.  Same queue discipline as the
 * reference: bit-identical outputs. */
int fgc_mesh_patch(const float* V_h, int32_t nv, const int32_t* F_h, int32_t nf, const int32_t* adj_h, int32_t K,
                   int32_t face_num, int32_t seed, float* v_out_h, int32_t v_cap, int32_t* f_out_h, int32_t* adj_out_h,
                   int32_t* v_old_h, int32_t* f_old_h, int32_t* n_v, int32_t* n_f);

/* Faces incident to every vertex = getVerticesFaces (utils.py:370-395), host.  faces_h [nf,3] int32 with -1 rows for
 * fake faces (skipped); v_faces_h [nv, k_v] receives the face (row) indices in face order, -1 padded.  -EINVAL if a
 * vertex is in more than k_v faces (the reference raises IndexError). */
int fgc_vertices_faces(const int32_t* faces_h, int32_t nf, int32_t nv, int32_t k_v, int32_t* v_faces_h);

/* Edge map = getEdgeMap (utils.py:91-183), host.  e_map_h [3*nf, 4] receives [v1, v2, f1, f2] per edge (f2 = -1
 * on a boundary), *n_edges the number of edges written; v_e_map_h [nv, max_edges] the edge ids incident to every
 * vertex in creation order, -1 padded.  Same visiting order as the reference, so both tables are bit-identical to
 * its output.  -EINVAL if a vertex has more than max_edges edges (the reference raises IndexError there). */
int fgc_edge_map(const uint32_t* faces_h, int32_t nf, int32_t nv, int32_t max_edges, int32_t* e_map_h,
                 int32_t* n_edges, int32_t* v_e_map_h);

/* ------------------------------------------------------------------------------------
 * Graph convolution  (replaces custom_conv2d, model.py:427-504, invariance-off branch,
 * with get_weight_assigments model.py:74-95 and get_patches model.py:380-405 fused in)
 *
 *   a_i = u x_i + c,  g_j = v x_j,  q_ik = softmax_m(a_i + g_j(i,k))
 *   y_i = (1/deg_i) sum_k sum_m q_ikm W0[m] x_j(i,k) + b [deg_i > 0]
 *
 * The input of node j is the channel concatenation [x0 | x1] of row (j >> shift) of each
 * source (shift = 2 reads a 4x-upsampled coarse tensor, model.py:817-825, without
 * materialising it; x1 = NULL for a single source; concat replaces tf.concat model.py:909,929).
 * act: 0 = none, 1 = leaky ReLU with `alpha` (model.py:828-830) applied to y.
 * y_pool (optional, may be NULL): max over each 4 consecutive rows of y (model.py:779-788).
 * ---------------------------------------------------------------------------------- */
/* One per-call override of a process-level option (fgc_set_option): `index` is the option's position in fgc_option_name's
 * enumeration.  A descriptor that carries a list (fgc_conv_desc.options) runs EVERY entry point it is passed to - workspace
 * queries, fgc_conv_uses_pairs, fgc_conv_pack, forward, backward, fgc_conv_bwd_reduce - with these values instead of the
 * process-level ones, for that descriptor only and on the calling thread only: two networks in one process (or two layers of
 * one network) can take different kernel forms without touching global state.  The same caveat as for fgc_set_option holds per
 * descriptor: keep a descriptor's list the same from its plan / pack calls to the calls that consume their results. */
typedef struct fgc_option_override {
    int32_t index;
    int32_t reserved;       /* 0 */
    int64_t value;
} fgc_option_override;

typedef struct fgc_conv_desc {
    int32_t n;              /* nodes of this level */
    int32_t nnz;            /* edges */
    const int32_t* rowptr;  /* [n+1] */
    const int32_t* col;     /* [nnz]; at least one readable entry (a level of nothing but edgeless nodes reads col[0]) */
    const float* x0;        /* [(n >> shift), c0] */
    const float* x1;        /* [(n >> shift), c1] or NULL */
    int32_t c0, c1;         /* cin = c0 + c1 */
    int32_t shift;          /* 0 or 2 */
    int32_t cout;
    const float* W0;        /* [M, cout, cin]  (model.py:430) */
    const float* b;         /* [cout]          (model.py:431) */
    const float* u;         /* [M, cin]        (model.py:432) */
    const float* c;         /* [M]             (model.py:433) */
    const float* v;         /* [M, cin]        (model.py:447) */
    int32_t bias_mask;      /* model.py:496-500 */
    int32_t act;
    float alpha;
    int32_t src_rows;       /* rows of x0/x1 to compute assignment logits for; 0 = n >> shift.  Larger when the
                               source tensors carry halo rows behind the owned ones (facet sharding) */
    int32_t max_deg;        /* max_i deg(i) if the caller knows it, else 0.  <= 24 (every reference K-list) enables
                               the producer/consumer kernels; 0 or larger falls back to the edge-chunking path */
    /* Partial forward calls (all zero = the whole layer in one call).  A facet-sharded caller computes the tiles
     * that gather owned rows only while the halo rows are still travelling, then the rest:
     *   call 1: tile_list = interior tiles, proj_rows = owned source rows
     *   call 2: tile_list = boundary tiles, proj_row0 = owned source rows, proj_rows = halo rows, FGC_CONV_PACKED
     * fgc_conv_bwd ignores these four fields (its split is in fgc_conv_bwd_io). */
    const int32_t* tile_list; /* device, [n_tiles]: indices of the 32-row output tiles to compute; NULL = all */
    int32_t n_tiles;          /* may be 0 with a non-NULL list: no conv launch, logits only */
    int32_t proj_row0;        /* assignment logits are computed for source rows [proj_row0, proj_row0 + proj_rows) */
    int32_t proj_rows;        /* 0 = all src_rows (proj_row0 must be 0), < 0 = none */
    int32_t flags;            /* FGC_CONV_PACKED */
    /* Optional, shift == 2 only: the pair graph of this level (fgc_pair_graph).  With it (and hc) the layer runs on its
     * COARSE source rows: h_P = W0 x_P once per coarse row (one [n/4, cin] x [cin, M*cout] product instead of a tile
     * product per fine node), y_i = (1/deg_i) sum_P mult_iP sum_m q_pPm h_Pm - the same sums as the fine form in another
     * order; fgc_conv_uses_pairs tells whether a descriptor qualifies.  All NULL / 0: the fine form. */
    const int32_t* pair_rowptr;  /* [n/4 + 1] */
    const int32_t* pair_col;     /* [n_pairs]: source row of the parent (< src_rows); at least one readable entry */
    const uint32_t* pair_mul;    /* [n_pairs]: four 8-bit multiplicities (fgc_pair_graph); at least one readable entry */
    int32_t n_pairs;
    int32_t max_pair_deg;        /* largest number of pairs of a block */
    int32_t max_pair_in_deg;     /* largest number of in-pairs of a coarse row (transposed pair graph); 0 = not known:
                                    forward only.  fgc_conv_bwd needs 1 .. 24 */
    float* hc;                   /* [src_rows (or n/4), M*cout], 16-byte aligned: the transformed coarse rows, written by
                                    fgc_conv_fwd and read again by fgc_conv_bwd (bf16 with FGC_CONV_BF16).  A partial forward
                                    call transforms the source rows [proj_row0, proj_row0 + proj_rows) only; with a tile_list
                                    of no tiles it stops there, without a tile_list it then computes every block (a
                                    facet-sharded caller: owned rows while the halo parents travel, then the rest) */
    const fgc_option_override* options;  /* HOST pointer, [n_options]: per-descriptor option values (see above); NULL = none */
    int32_t n_options;
    int32_t reserved1;
    uint64_t packed_layout;      /* 0, or fgc_conv_layout_id(this descriptor) as it read when the operands in the workspaces
                                    were packed: a call told FGC_CONV_PACKED then returns FGC_EINVAL if the option values of
                                    the moment select another operand layout, instead of multiplying by the wrong one */
} fgc_conv_desc;

/* the workspace still holds the packed operands of the previous call with this descriptor: skip the packing */
#define FGC_CONV_PACKED 1
#define FGC_CONV_DEFER_REDUCE 2   /* fgc_conv_bwd_io.flags: stage 8 leaves its partial sums for fgc_conv_bwd_reduce */
#define FGC_CONV_DEFER_DW 16      /* fgc_conv_bwd_io.flags, with FGC_CONV_DEFER_REDUCE: stage 8 does not launch the layer's
                                   * weight-gradient GEMM either; fgc_conv_bwd_reduce runs the GEMMs of all such layers in one
                                   * launch per kernel form (same slabs, bit-identical gradients).  The layer's r (a first layer
                                   * over a narrow input: ds and its saved aggregates), its inputs x0 / x1 and its workspace must
                                   * then stay untouched until that call: a caller that shares r between layers cannot use it */
#define FGC_CONV_R_PAD 32         /* fgc_conv_bwd_io.flags: the rows of r are padded to whole 128-byte lines - row stride
                                     fgc_conv_r_ld(cout, 1, bf16) elements instead of M*cout + 24 (columns unchanged: M*cout
                                     aggregate columns, then da | dg; the pad columns are never read).  Read only when
                                     fgc_conv_bwd_io.r_ld == 0; a caller that sets r_ld states the stride once, with the
                                     buffer, and need not repeat the flag in every staged call */
#define FGC_CONV_SAVE_Z 4         /* fgc_conv_desc.flags, first layer over a narrow input (cin <= 8): the forward pass
                                  * leaves the aggregates z [n, roundup4(9*cin)] in its workspace (sized for it by
                                  * fgc_conv_workspace_bytes when the flag is set) so that the backward pass, given
                                  * fgc_conv_bwd_io.z_saved, does not recompute them for the weight gradient */

#define FGC_CONV_BF16 8           /* fgc_conv_desc.flags: bf16 STORAGE / fp32 accumulate (a build extension: the reference is
                                  * fp32 only, train.py:409-427).  x0, x1, y, y_pool and, in fgc_conv_bwd, dy, ds, r, dx0 and
                                  * dx1 point to bf16 (uint16_t) tensors of the same shapes; the gathers move half the
                                  * bytes and the dense contractions run on v_mfma_f32_16x16x32_bf16 with fp32
                                  * accumulation.  Logit tables (ag, dag), per-edge d-logits (dl), parameters and
                                  * parameter gradients stay fp32; the weight-gradient reduction over nodes multiplies the
                                  * bf16-stored operands on the fp32 MFMA (exact products, fp32 sums).  Supported for the
                                  * shapes of the network (widths that are multiples of 32, degrees <= 24); a narrow first
                                  * layer (cin <= 8) keeps its fp32 input x0 and ds, and stores y / y_pool as bf16.
                                  * Same flag in fgc_conv_bwd_io.flags is not needed: the descriptor's flag rules. */

/* bytes of scratch the conv entry points need for this descriptor (packed weights) */
size_t fgc_conv_workspace_bytes(const fgc_conv_desc* d);

/* forward.  ag [(n >> shift), FGC_AG_LD] receives the assignment logits (kept for backward).
 * y [n, cout]; y_pool [n/4, cout] or NULL. */
int fgc_conv_fwd(const fgc_conv_desc* d, float* ag, float* y, float* y_pool, void* workspace,
                 size_t workspace_bytes, void* stream);

/* backward.  Transposed CSR required.  dy is the gradient w.r.t. the POST-activation output y
 * (y itself is passed to recover the leaky-ReLU mask).  Scratch the caller provides:
 *   ds   [n, cout]           dy * lrelu'(y) / deg
 *   dl   [nnz, FGC_DL_LD]    per-edge d(logit)
 *   dag  [n, FGC_AG_LD]      d a (0..8) | d g (12..20) per node of this level
 *   r    [n, M*cout + 24]    backward-side aggregate, then da | dg of the node (one GEMM gives dW0, du and dv)
 * Outputs: dW0,db,du,dc,dv (overwritten); dx0/dx1 [(n >> shift), c0/c1] either overwritten
 * (accumulate = 0) or added to (accumulate = 1); dx pointers may be NULL (conv1: no input grad). */
typedef struct fgc_conv_bwd_io {
    const int32_t* trowptr; /* [n+1] */
    const int32_t* tcol;    /* [nnz] */
    const int32_t* tedge;   /* [nnz] */
    int32_t max_in_deg;     /* max in-degree of the transposed graph if known, else 0 (see max_deg) */
    int32_t stages;         /* 0 = whole backward.  Otherwise a bit mask, so that a facet-sharded caller can exchange
                               halo rows between the pieces: 1 = ds/db, 2 = logits (dl, da, dc), 4 = data kernel
                               (r, dg, dx) over data_tile_list, 8 = weight gradients (dW0, du, dv; needs every r and
                               dg row).  ds then has rows for halo sources behind the n owned ones, and dl rows for
                               incoming cross-shard edges behind the nnz owned ones. */
    const float* ag;        /* saved by forward */
    const float* y;         /* forward output (post activation) */
    const float* dy;        /* [n, cout] */
    float* ds;
    float* dl;
    float* dag;
    float* r;
    float* dx0;
    float* dx1;
    int32_t accumulate0, accumulate1;
    float* dW0;
    float* db;
    float* du;
    float* dc;
    float* dv;
    const int32_t* data_tile_list; /* device, [n_data_tiles]: 32-row tiles stage 4 computes; NULL = all.  Tiles whose
                                      in-edges all come from owned rows need neither halo rows of ds nor remote dl.  Pair
                                      form: tiles of the n / 4 COARSE rows the data kernel runs over (those whose in-pairs
                                      all have owned parents need no incoming dt / dl row) */
    int32_t n_data_tiles;
    int32_t flags;                 /* FGC_CONV_PACKED: the operands are already packed (an earlier stage call, or
                                    * fgc_conv_pack); FGC_CONV_DEFER_REDUCE: see fgc_conv_bwd_reduce */
    const float* z_saved;          /* optional: the workspace of the forward call made with FGC_CONV_SAVE_Z */
    /* optional: the layer's output also went through the 4:1 max pooling (custom_binary_tree_pooling, model.py:779-788)
     * and the pooled tensor's gradient is still to be folded in: stage 1 then uses
     *   dy_i + [y_i == pool_y_(i/4)] * pool_dy_(i/4) / #{rows of the group equal to the maximum}
     * instead of dy_i (tf.reduce_max's gradient, as fgc_pool4_bwd computes it) - no separate pass over dy.
     * pool_y, pool_dy: [n / 4, cout], the pooled output and its gradient (bf16 with FGC_CONV_BF16). */
    const float* pool_y;
    const float* pool_dy;
    /* pair form (fgc_conv_desc.pair_rowptr): the transposed pair graph and scratch for the per-pair output gradients
     * dt_pP = sum_children mult_iP dy_i / deg_i.  dl then holds one row per PAIR, r one row per COARSE row
     * ([n/4, M*cout + 24]); ds is not used. */
    const int32_t* tpair_rowptr; /* [n/4 + 1] */
    const int32_t* tpair_col;    /* [n_pairs]: block p of the in-pair */
    const int32_t* tpair_edge;   /* [n_pairs]: its pair id */
    float* dt;                   /* [n_pairs (+ incoming cross-shard pairs), cout], 16-byte aligned (bf16 with
                                    FGC_CONV_BF16): stage 1|2 writes the rows of the owned pairs, stage 4 gathers the rows the
                                    transposed pair graph names (tpair_edge), like dl */
    int32_t r_ld;                /* row stride of r in elements (fp32 floats / bf16 halves), a property of the BUFFER: stage 4
                                    writes with it, stage 8 and fgc_conv_bwd_reduce read with it, whatever `flags` holds in
                                    each of those calls.  0 = derive it from flags (FGC_CONV_R_PAD set or not) in every call,
                                    as ABI 103 did.  Otherwise >= M*cout + 24 and congruent to it modulo 4 (bf16: modulo 8) -
                                    fgc_conv_r_ld() returns the two strides the kernels are tuned for. */
    int32_t reserved0;
} fgc_conv_bwd_io;

size_t fgc_conv_bwd_workspace_bytes(const fgc_conv_desc* d);
/* row stride of fgc_conv_bwd_io.r in elements (fp32: floats, FGC_CONV_BF16: 2-byte halves): M*cout + 24, or with
 * padded != 0 (FGC_CONV_R_PAD) that rounded up to a multiple of 128 bytes */
int32_t fgc_conv_r_ld(int32_t cout, int32_t padded, int32_t bf16);
/* 1 if a staged (facet-sharded) backward of this layer needs the halo rows of ds and the d-logits of incoming
 * cross-shard edges between its stages; 0 for a first layer over a narrow input (dx0 == NULL, cin <= 8), whose
 * parameter gradients are sums over the owned nodes only (stages 1, 2, 8; stage 4 is empty). */
int fgc_conv_bwd_needs_exchange(const fgc_conv_desc* d, const fgc_conv_bwd_io* io);
/* 1 if fgc_conv_fwd / fgc_conv_bwd run this descriptor in the pair form.  All of:
 *   - pair_rowptr, pair_col, pair_mul and hc given; shift == 2; ONE source (x1 == NULL, c1 == 0); n % 4 == 0;
 *   - cin (= c0) 32, 64 or 128, cout 32 or 64; fp32 or bf16 storage (FGC_CONV_BF16: hc and dt are then bf16);
 *   - n_pairs > 0, max_pair_deg > 0, 0 <= max_pair_in_deg <= 24 (the data-gradient kernel's edge-slot limit);
 *   - rows of hc (src_rows, or n / 4) < 2^24 and rows * 9 * cout * 4 < 2^32; n_pairs < 2^24 - 2^20 and
 *     n_pairs * cout * 4 < 2^32 (row ids go through 24-bit multiplies and 32-bit buffer offsets; the margin leaves room for
 *     a facet-sharded rank's incoming cross-shard pairs behind its own in dt);
 *   - x0 and hc 16-byte aligned;
 *   - the whole layer in one call, OR one of the two partial forward calls a facet-sharded caller makes: "transform +
 *     logits of the source rows [proj_row0, proj_row0 + proj_rows) only" (tile_list != NULL with n_tiles == 0) and "the rest
 *     of the source rows, then every block" (tile_list == NULL, proj_row0 / proj_rows naming the rest).  A tile list WITH
 *     tiles (an interior / boundary split of the blocks) selects the fine form;
 *   - options NO_PAIRS, NO_W8 and NO_W8FAST all 0 (fgc_set_option; the last two take the pair form's data-gradient kernel
 *     away).
 * Anything else: 0, and the layer runs in the fine form without an error.  fgc_conv_bwd of a pair-form layer REQUIRES the
 * transposed pair graph and dt in its io.  Ranks of a facet-sharded job must agree on the answer per layer (they exchange
 * different tensors in the two forms): decide it on the GLOBAL pair graph (largest in-degree, pair counts), not per rank. */
int fgc_conv_uses_pairs(const fgc_conv_desc* d);
/* The GRAPH-dependent limits of the list above alone (in-pairs per coarse row, row and pair counts against the 24-bit row ids
 * and 32-bit buffer offsets of the pair kernels), for counts that need not be a descriptor's: a facet-sharded job evaluates
 * them on the GLOBAL pair graph so that every rank decides alike (fgc_conv_uses_pairs applies the same function to the
 * descriptor's own counts).  rows: coarse source rows; 1 = allowed. */
int fgc_conv_pairs_allowed(int64_t rows, int64_t n_pairs, int32_t max_pair_in_deg, int32_t cout);
/* Which packed-operand layouts the option values of THIS moment (process options, then the descriptor's own overrides)
 * select for the descriptor - first-layer path or not, pair form or not, d-logits operand as fp32 or as bf16 split planes,
 * storage type.  Never 0.  Operands packed ahead of their use (fgc_conv_pack, or an earlier call) are only valid while this
 * value stays what it was: store it in fgc_conv_desc.packed_layout and the FGC_CONV_PACKED calls check it (packed_layout is
 * not part of the value). */
uint64_t fgc_conv_layout_id(const fgc_conv_desc* d);
int fgc_conv_bwd(const fgc_conv_desc* d, const fgc_conv_bwd_io* io, void* workspace, size_t workspace_bytes,
                 void* stream);
/* Which kernel form every launch of fgc_conv_fwd / fgc_conv_bwd takes for this descriptor (and this io), under the option
 * values in force (process options, then the descriptor's own overrides), as ONE line of space-separated key=value pairs in
 * buf.  Host only: launches nothing and dereferences no device pointer (addresses are read for their alignment and for being
 * NULL).  Every value is the answer of the function the launch itself branches on.  io == NULL: the forward keys and what the
 * backward plan decides without the call's pointers.  Returns the length written (without the NUL), FGC_EINVAL if the
 * descriptor is invalid or buf too small (512 bytes are enough).  Keys (k2_* / k3 / ds and the starred k1 keys need io):
 *   fwd        pair | narrow | w8 (eight-wave kernel) | tiled (conv_fwd_kernel)
 *   fwd_mma    narrow only: per-node products on the matrix cores
 *   fwd_fast fwd_slots fwd_nt fwd_bfm   w8: fast-shape kernel; edge slots 16 / 24; nodes per workgroup 16 / 32; bf16 matrix-pipe
 *              aggregation (0 / 24 / 32 / 0 for the other kinds)
 *   fwd_vec4   16-byte input rows (conv_fwd_kernel<vec4> against <scalar>; the blocking logit kernel likewise)
 *   proj       logit-table kernel: pair | narrow | bf16 | stream | block
 *   ds         who computes s = dy lrelu'(y) / deg and the db partials: pair | fused (d-logits prologue) | narrow-fused |
 *              vec (ds_db_vec_kernel) | scalar (ds_db_kernel)
 *   k1         d-logits kernel: pair | narrow | bf16 | deep | mfma | valu;  k1_mma* (narrow only)
 *   k1_long k1_half k1_split k1_nodes   17..24 edge slots; 16-node workgroups; dz GEMM on split bf16 operands; nodes per workgroup
 *   k1_okg* k1_aglobal* k1_vec4*        deep: compile-time column groups (0 = any width); ds tile read from global memory;
 *              mfma / valu: 16-byte gathers
 *   k2         data-gradient kernel: none (narrow first layer without dx) | w8 | tiled (conv_bwd_data_kernel)
 *   k2_fast k2_slots k2_nt k2_bfm k2_vec4   as for fwd (tiled: vec4 = 16-byte rows of ds and r)
 *   k2_chunks  ceil(max in-degree / 24): passes of the tiled kernel over a node's in-edge list (0: degree not stated)
 *   k3         weight-gradient GEMM: stream2 | stream4 | stream2_bf | stream4_bf | bf16_4 | bf16_2 | plain_v4 | plain | narrow
 *   k3_slabs k3_rows   slabs of the GEMM and rows per slab (the last slab holds the rest)
 *   nb_db n_dc layout_id   db / dc partial-sum slots; fgc_conv_layout_id */
int fgc_conv_forms(const fgc_conv_desc* d, const fgc_conv_bwd_io* io, char* buf, int32_t buf_bytes);

/* Extra jobs of fgc_conv_pack's launch (each part optional: rot_x == NULL / mlp_W1 == NULL skips it). */
typedef struct fgc_pack_extra {
    /* rot_y[r, 3v:3v+3] = R rot_x[r, 3v:3v+3] for rot_rows rows of rot_vecs 3-vectors (fgc_rotate_rows) */
    const float* rot_x;
    float* rot_y;
    const float* rot_R;         /* [9] on the device */
    int64_t rot_rows;
    int32_t rot_vecs;
    /* optional (rot_vecs <= 2): the assignment-logit table of the layer that reads rot_y (the network's first layer:
     * rot_ag [rot_rows, 24] = what its fgc_conv_fwd would compute from u [9, 3 rot_vecs], c [9], v [9, 3 rot_vecs]) in the
     * same pass; that layer's forward call then sets proj_rows = -1.  Same arithmetic as the layer's own table launch. */
    float* rot_ag;
    const float* rot_u;
    const float* rot_c;
    const float* rot_v;
    /* the MLP whose operands are packed: W1 [cin, hidden], W2 [hidden, cout] (bf16 backward only), n rows.  mlp_fwd_ws /
     * mlp_bwd_ws are the workspaces later handed to fgc_mlp_fwd / fgc_mlp_bwd (mlp_bf16 != 0: to the _bf16 forms) with
     * FGC_MLP_PACKED; they must stay untouched in between, so the two calls need workspaces of their own.  Either may
     * be NULL. */
    int32_t mlp_bf16;
    const float* mlp_W1;
    const float* mlp_W2;
    int32_t mlp_n, mlp_cin, mlp_hidden, mlp_cout;
    void* mlp_fwd_ws;
    void* mlp_bwd_ws;
} fgc_pack_extra;

/* Whole-network helpers for a caller that runs the same `count` layers every step (train.py:558-575 runs the graph of
 * model.py:853-941 once per iteration) and gives every layer a workspace of its own that stays untouched from the
 * first call of a step to the last: the per-layer housekeeping launches (each costs about 5 us on an idle MI355X
 * whatever its size) collapse into one.
 *
 * fgc_conv_pack: the packed weight operands of all layers in ONE launch - forward operands into fwd_ws[i], the two
 * backward operands into bwd_ws[i] (either array, or single entries, may be NULL to skip; ios may be NULL, it only
 * tells which layer takes the narrow first-layer path and has nothing to pack).  Call it after the weights change;
 * then pass FGC_CONV_PACKED in fgc_conv_desc.flags / fgc_conv_bwd_io.flags.
 * `extra` (may be NULL): the step's other housekeeping in the same launch - the rotation of the input rows
 * (train.py:563-565, what fgc_rotate_rows does) and the operands of the network's per-facet MLP, which the fgc_mlp_*
 * entry points then take with FGC_MLP_PACKED.  count may be 0 with descs NULL.
 *
 * fgc_conv_bwd_reduce: (layers with FGC_CONV_DEFER_DW: first their weight-gradient GEMMs, grouped.)  With
 * FGC_CONV_DEFER_REDUCE in fgc_conv_bwd_io.flags stage 8 leaves the partial sums of the
 * parameter gradients in the layer's workspace; this call sums them for all layers in two launches, in the same
 * fixed order as the per-layer path (bit-identical gradients). */
int fgc_conv_pack(const fgc_conv_desc* const* descs, const fgc_conv_bwd_io* const* ios, void* const* fwd_ws,
                  void* const* bwd_ws, int32_t count, const fgc_pack_extra* extra, void* stream);
int fgc_conv_bwd_reduce(const fgc_conv_desc* const* descs, const fgc_conv_bwd_io* const* ios, void* const* bwd_ws,
                        int32_t count, void* stream);

/* ------------------------------------------------------------------------------------
 * Per-facet MLP  cin -> hidden -> cout with leaky ReLU in between
 * (replaces lrelu(custom_lin(x,1024)) -> custom_lin(.,3), model.py:763-769,937-941; the
 * [n, hidden] tensor never leaves the CU).  W1 [cin, hidden], b1 [hidden], W2 [hidden, cout], b2 [cout].
 * abs_partial (optional): per-workgroup partial sums of |y| for normalizeTensor's global mean;
 * needs fgc_mlp_num_partials(n) floats.
 * Everything is fp32 in and out.  For 32- and 64-wide inputs fgc_mlp_fwd multiplies x W1 on the bf16 matrix pipe with
 * three-term operand splits (v = bf16(v) + bf16(v - v0) + bf16(v - v0 - v1); six exact partial products per product,
 * fp32 accumulation): as close to a float64 reference as the fp32 MFMA kernel it replaces (1.7e-7 vs 2.0e-7 on outputs
 * of size 1).  FGC_NO_MLP_SPLIT=1 in the environment keeps the fp32 MFMA.  alpha must be in [0, 1].
 * hidden: a multiple of 64 (forward) / 256 (backward); cout 1 ... 4; cin 1 ... 128.  The workspace must be 16-byte aligned;
 * x, dx and b1 need not be (a call whose rows, dx or b1 are not takes the fp32 MFMA: fgc_mlp_forms tells).
 * flags: FGC_MLP_PACKED = the workspace already holds this call's weight operands (fgc_conv_pack with an
 * fgc_pack_extra naming it, same W1 / W2 / shape, nothing written to it since): the call skips its own pack launch.
 * ---------------------------------------------------------------------------------- */
#define FGC_MLP_PACKED 1
/* The MLP's counterpart of fgc_conv_layout_id: which operand layouts the option values of this moment select for the shape
 * (1 ... 255; bf16 != 0: the _bf16 entry points).  OR FGC_MLP_LAYOUT(id as it read when the workspace was packed) into the
 * flags of an FGC_MLP_PACKED call and the call returns FGC_EINVAL if the options moved in between; without it nothing is
 * checked. */
#define FGC_MLP_LAYOUT(id) ((int32_t)(id) << 8)
int32_t fgc_mlp_layout_id(int32_t cin, int32_t hidden, int32_t cout, int32_t bf16);
int32_t fgc_mlp_num_partials(int32_t n);
size_t fgc_mlp_workspace_bytes(int32_t cin, int32_t hidden, int32_t cout);
size_t fgc_mlp_bwd_workspace_bytes(int32_t n, int32_t cin, int32_t hidden, int32_t cout);
int fgc_mlp_fwd(const float* x, int32_t n, int32_t cin, int32_t hidden, int32_t cout, const float* W1,
                const float* b1, const float* W2, const float* b2, float alpha, float* y, float* abs_partial,
                int32_t flags, void* workspace, size_t workspace_bytes, void* stream);
/* dW1,db1,dW2,db2 overwritten; dx [n, cin] overwritten. */
int fgc_mlp_bwd(const float* x, const float* dy, int32_t n, int32_t cin, int32_t hidden, int32_t cout,
                const float* W1, const float* b1, const float* W2, float alpha, float* dx, float* dW1,
                float* db1, float* dW2, float* db2, int32_t flags, void* workspace, size_t workspace_bytes, void* stream);

/* The same MLP with bf16-STORED activations (companion of FGC_CONV_BF16; a build extension, the reference is fp32 only:
 * train.py:409-427).  x [n, cin] and dx [n, cin] are bf16 (uint16_t) tensors, cin in {32, 64, 128} (backward: 32, 64),
 * hidden a multiple of 256; parameters, their gradients, y and dy stay fp32.  The products with the hidden layer run on
 * v_mfma_f32_16x16x32_bf16 with fp32 accumulation, everything else in fp32. */
size_t fgc_mlp_bf16_workspace_bytes(int32_t cin, int32_t hidden, int32_t cout);
size_t fgc_mlp_bwd_bf16_workspace_bytes(int32_t n, int32_t cin, int32_t hidden, int32_t cout);
int fgc_mlp_fwd_bf16(const void* x, int32_t n, int32_t cin, int32_t hidden, int32_t cout, const float* W1,
                     const float* b1, const float* W2, const float* b2, float alpha, float* y, float* abs_partial,
                     int32_t flags, void* workspace, size_t workspace_bytes, void* stream);
int fgc_mlp_bwd_bf16(const void* x, const float* dy, int32_t n, int32_t cin, int32_t hidden, int32_t cout,
                     const float* W1, const float* b1, const float* W2, float alpha, void* dx, float* dW1, float* db1,
                     float* dW2, float* db2, int32_t flags, void* workspace, size_t workspace_bytes, void* stream);

/* Which kernel form the MLP entry points (bf16 != 0: the _bf16 ones) take for a shape under the options in force and with
 * the pointers of a call, as ONE line of space-separated key=value pairs: the plan the launches follow, printed.  Launches
 * nothing and follows no pointer: x, dx, b1, fwd_ws, bwd_ws are looked at for their alignment only, NULL stands for an aligned
 * pointer.  Returns the length written (without the NUL), FGC_EINVAL if buf is NULL or too small (512 bytes are enough).
 *   fwd        f32 (fp32 MFMA) | split (three-term bf16 operand splits) | bf16 | none (fgc_mlp_fwd[_bf16] refuses the call)
 *   fwd_ks fwd_co fwd_kpad fwd_gx   template selector (f32: k groups known at compile time, 0 = any; else cin / 32); output
 *              columns carried in registers; f32: input channels padded to the k group; workgroups
 *   bwd        f32 | split | bf16 | none
 *   bwd_mt bwd_ctw bwd_co   template selectors: input-channel tiles of 16; f32: column tiles per wave; output columns
 *   bwd_slabs bwd_dx_slabs bwd_dx_gx bwd_gx bwd_gy   parameter-gradient slabs (= row walkers); f32: dx slabs; workgroups of
 *              the dx kernel (0: one fused kernel); grid of the parameter-gradient kernel
 *   fwd_shape bwd_shape   the form the shape alone selects: what fgc_conv_pack leaves in the workspace
 *   layout     fgc_mlp_layout_id */
int fgc_mlp_forms(int32_t n, int32_t cin, int32_t hidden, int32_t cout, int32_t bf16, const void* x, const void* dx,
                  const void* b1, const void* fwd_ws, const void* bwd_ws, char* buf, int32_t buf_bytes);

/* ------------------------------------------------------------------------------------
 * Element-wise / reduction ops
 * ---------------------------------------------------------------------------------- */
/* leaky ReLU (model.py:828-830), forward and backward from the OUTPUT y */
int fgc_lrelu_fwd(const float* x, float* y, int64_t count, float alpha, void* stream);
int fgc_lrelu_bwd(const float* y, const float* dy, float* dx, int64_t count, float alpha, void* stream);
/* 4:1 max pooling over consecutive rows (model.py:779-788, steps = 2) */
int fgc_pool4_fwd(const float* x, float* y, int32_t n_out, int32_t c, void* stream);
/* gradient of max pooling, split evenly over ties (tf.reduce_max semantics).  accumulate: dx += */
int fgc_pool4_bwd(const float* x, const float* y, const float* dy, float* dx, int32_t n_out, int32_t c,
                  int32_t accumulate, void* stream);
/* the same on bf16 tensors (all four; FGC_CONV_BF16 storage) */
int fgc_pool4_bwd_bf16(const void* x, const void* y, const void* dy, void* dx, int32_t n_out, int32_t c,
                       int32_t accumulate, void* stream);
/* 1:4 upsampling by repetition (model.py:817-825) and its gradient (sum of 4 rows) */
int fgc_upsample4_fwd(const float* x, float* y, int32_t n_in, int32_t c, void* stream);
int fgc_upsample4_bwd(const float* dy, float* dx, int32_t n_in, int32_t c, int32_t accumulate, void* stream);

/* custom_binary_tree_pooling 'max' (model.py:779-788) and custom_upsampling (model.py:817-825) for any steps:
 * group = 2^steps consecutive rows per pooled row (the 4:1 forms above are group = 4).  Pooling gradient = tf.reduce_max's:
 * split evenly over the entries equal to the maximum. */
int fgc_pool_fwd(const float* x, float* y, int32_t n_out, int32_t c, int32_t group, void* stream);
int fgc_pool_bwd(const float* x, const float* y, const float* dy, float* dx, int32_t n_out, int32_t c, int32_t group,
                 int32_t accumulate, void* stream);
int fgc_upsample_fwd(const float* x, float* y, int32_t n_in, int32_t c, int32_t group, void* stream);
int fgc_upsample_bwd(const float* dy, float* dx, int32_t n_in, int32_t c, int32_t group, int32_t accumulate, void* stream);

/* custom_lin (model.py:763-769) on its own: y [n, cout] = x [n, cin] W [cin, cout] + b, and its gradients
 * (dx may be NULL; dW [cin, cout], db [cout]; the sum over the n rows is split over workgroups and added in a fixed order).
 * Exact fp32 products on v_mfma_f32_16x16x4_f32.  The network's own two linear layers are fgc_mlp_fwd / fgc_mlp_bwd (hidden
 * layer kept on chip); this is for callers that compose custom_lin -> lrelu -> custom_lin themselves. */
size_t fgc_lin_bwd_workspace_bytes(int32_t n, int32_t cin, int32_t cout);
int fgc_lin_fwd(const float* x, int32_t n, int32_t cin, int32_t cout, const float* W, const float* b, float* y, void* stream);
int fgc_lin_bwd(const float* x, const float* dy, int32_t n, int32_t cin, int32_t cout, const float* W, float* dx, float* dW,
                float* db, void* workspace, size_t workspace_bytes, void* stream);

/* normalizeTensor (utils.py:1700-1715).  scratch: 2 + fgc_norm_num_partials(n) floats.
 * If abs_partial/num_partials come from fgc_mlp_fwd they are used for the global mean,
 * otherwise pass NULL/0 and the op reduces |x| itself. */
int32_t fgc_norm_num_partials(int32_t n);
int fgc_normalize_fwd(const float* x, int32_t n, const float* abs_partial, int32_t num_partials, float* y,
                      float* scratch, void* stream);
int fgc_normalize_bwd(const float* x, const float* dy, int32_t n, float* dx, float* scratch, void* stream);
/* The same op in pieces, for a tensor whose rows are sharded over ranks (the global mean and its gradient need one
 * scalar all-reduce each, done by the caller between the pieces):
 *   apply:        y = normalise rows of x with scratch[0] = mean|x| + 1e-5 supplied by the caller
 *   bwd_partial:  dx <- d(x/s) per row, partial[0..fgc_norm_num_partials(n)) <- block sums of <d(x/s), x>
 *   bwd_apply:    dx <- dx / s + sign(x) * scratch[1] / total_count, scratch[1] = -(global sum) / s^2 from the caller */
int fgc_normalize_apply(const float* x, int32_t n, const float* scratch, float* y, void* stream);
int fgc_normalize_bwd_partial(const float* x, const float* dy, int32_t n, const float* scratch, float* dx,
                              float* partial, void* stream);
int fgc_normalize_bwd_apply(const float* x, int32_t n, float total_count, const float* scratch, float* dx,
                            void* stream);

/* angular loss on sampled rows (train.py:509-517 gather + faceNormalsLoss train.py:1272-1294).
 * fn, gt [n,3]; sample_ind int32 [ns]; loss_out [2] = {loss in degrees, number of real rows}.
 * bwd: dfn [n,3] is zero-filled then receives d loss / d fn (scaled by dloss). */
int fgc_angular_loss_fwd(const float* fn, const float* gt, const int32_t* sample_ind, int32_t ns, float* loss_out,
                         void* stream);
int fgc_angular_loss_bwd(const float* fn, const float* gt, const int32_t* sample_ind, int32_t ns, int32_t n,
                         const float* loss_out, float dloss, float* dfn, void* stream);

/* The loss end of one training step in TWO launches: normalizeTensor on the network output (utils.py:1700-1715), the
 * rotation of the ground truth (train.py:439-451, applied to the sampled rows only), the sampled angular loss
 * (train.py:509-517, faceNormalsLoss train.py:1272-1294), its gradient, and normalizeTensor's gradient - what
 * fgc_normalize_fwd + fgc_rotate_rows + fgc_angular_loss_fwd / _bwd + fgc_normalize_bwd do in seven.
 *   y [n,3]: the network output; abs_partial / num_partials: the partial sums of |y| that fgc_mlp_fwd leaves;
 *   gt [n,3]: UNROTATED ground truth; R: device pointer to 9 floats or NULL (identity); sample_ind int32 [ns];
 *   gacc [n,3]: scratch that must be ZERO on entry and is zero again when the call has run (only sampled rows are ever
 *   touched: the caller zero-fills it once, when it allocates it);
 *   n_conv [n,3] (may be NULL): the normalised rows; dy [n,3]: d loss / d y; loss_out [2] = {loss in degrees, real rows};
 *   scratch: fgc_loss_step_scratch_floats(ns) floats ([0] = mean|y| + eps, [1] = d loss / d of it, then one partial
 *   triple per 256 samples).
 * Same arithmetic per row as the separate entry points; sums over the samples instead of over all rows, and the division
 * by the number of real samples is applied once, at the end. */
int32_t fgc_loss_step_scratch_floats(int32_t ns);
int fgc_loss_step(const float* y, int32_t n, const float* abs_partial, int32_t num_partials, const float* gt,
                  const float* R, const int32_t* sample_ind, int32_t ns, float* gacc, float* n_conv, float* dy,
                  float* loss_out, float* scratch, void* stream);

/* The same for a FACET-SHARDED step (the rows of y are split over ranks): three calls with the step's
 * two scalar all-reduces between them.  sums: fgc_loss_shard_floats(ns_total) floats, ns_total = the number of samples of
 * the WHOLE step (it sizes the partial table identically on every rank); total_count = 3 x the rows of the whole tensor.
 *   1. fgc_loss_shard_abs_sum: sums[0] = this rank's sum of |y| (from fgc_mlp_fwd's partials)   -> ALL-REDUCE sums[0:1]
 *   2. fgc_loss_shard_samples: this rank's samples (LOCAL row ids, ns_local may be 0) -> gacc rows and the partial table
 *      sums[4 + 3 b] = {sum of angles, real samples, sum(d xs . y)} per 256 samples             -> ALL-REDUCE sums[4:]
 *   3. fgc_loss_shard_rows: dy, n_conv for the local rows; loss_out = the loss of the whole step; gacc zero again */
int32_t fgc_loss_shard_floats(int32_t ns_total);
int fgc_loss_shard_abs_sum(const float* abs_partial, int32_t num_partials, float* sums, void* stream);
int fgc_loss_shard_samples(const float* y, float total_count, const float* gt, const float* R, const int32_t* sample_local,
                           int32_t ns_local, int32_t ns_total, float* gacc, float* sums, void* stream);
int fgc_loss_shard_rows(const float* y, int32_t n_local, float total_count, int32_t ns_total, float* sums, float* gacc,
                        float* n_conv, float* dy, float* loss_out, void* stream);

/* random-rotation augmentation (train.py:439-451): every 3-vector v of every row becomes R v.
 * R: DEVICE pointer to 9 floats (row major; kept on the device so that a captured hipGraph can be
 * replayed with a new rotation).  vecs = channels / 3. */
int fgc_rotate_rows(const float* x, float* y, int32_t n, int32_t vecs, const float* R, void* stream);

/* TensorFlow-1 Adam over one flat parameter buffer (train.py:520, tf.train.AdamOptimizer defaults:
 * lr_t = lr*sqrt(1-b2^t)/(1-b1^t); p -= lr_t*m/(sqrt(v)+eps)).  t is 1-based. */
int fgc_adam_step(float* p, const float* g, float* m, float* v, int64_t count, int32_t t, float lr, float b1,
                  float b2, float eps, void* stream);

/* inference epilogue (train.py:115-121,136; utils.py:26-35): out[f] = normalize^2(n_conv[perm[f]]), f < num_faces */
int fgc_infer_epilogue(const float* n_conv, const int32_t* perm, int32_t num_faces, float* out, void* stream);

/* halo pack / unpack for facet sharding: dst[i] = src[idx[i]] rows of width c */
int fgc_gather_rows(const float* src, const int32_t* idx, int32_t count, int32_t c, float* dst, void* stream);
int fgc_scatter_add_rows(const float* src, const int32_t* idx, int32_t count, int32_t c, float* dst, void* stream);

/* Several row copies in ONE launch: the pack and the unpack side of a grouped halo exchange.  A sharded
 * step sends the halo rows of up to three tensors to every peer at once; packing them per (tensor, peer) into the send
 * buffer of one all-to-all, and copying what arrives into the halo tails of the tensors, is one call each instead of a
 * launch per piece.  Job j:  dst_j[i, 0..width) = src_j[(idx_j ? idx_j[i] : i), 0..width)  for i < rows.
 * Rows are `width` dwords (a bf16 row of C channels is C / 2 dwords).  At most FGC_ROW_JOBS_MAX jobs; `jobs` is a host
 * array read before the call returns.  Jobs must not overlap each other's destinations. */
#define FGC_ROW_JOBS_MAX 32
typedef struct fgc_row_job {
    const float* src;
    const int32_t* idx;       /* device, or NULL: rows are consecutive in src */
    float* dst;
    int32_t rows, width;
} fgc_row_job;
int fgc_copy_rows_jobs(const fgc_row_job* jobs, int32_t njobs, void* stream);

/* Vertex update from denoised normals = update_position2 (train.py:1467-1557; called with 60 iterations and
 * lambda = 1/18 by inferNetOld, train.py:129-139).  Jacobi iterations
 *   x_i <- x_i + lambda * sum_{edges e = (i,j,f1,f2) of i} sum_{f in {f1,f2}} n_f (n_f . (x_j - x_i))
 * x [nv,3] input positions, normals [nf,3], e_map [ne,4], v_e_map [nv,max_edges] (device copies of fgc_edge_map's
 * output).  x_out [nv,3] receives the result, tmp [nv,3] is scratch; x may alias neither.  iters >= 0. */
int fgc_vertex_update(const float* x, float* x_out, float* tmp, int32_t nv, const float* normals, int32_t nf,
                      const int32_t* e_map, int32_t ne, const int32_t* v_e_map, int32_t max_edges, int32_t iters,
                      float lambda, void* stream);

/* Vertex update along a per-vertex direction = update_position_with_depth (train.py:1561-1665): fgc_vertex_update with
 * every contribution projected onto the direction d_i of its vertex (a vertex of a depth scan is a sample along a viewing
 * ray and may move along that ray only).  dirs [n_dirs,3]: d_i is row i when n_dirs == nv, the one row when n_dirs == 1;
 * any other n_dirs is FGC_EINVAL.  d is used as given - unit or not, nothing is normalised: the rule is sum (u . d) d.
 * Per Jacobi iteration and vertex, with u_s = n_f1 (n_f1 . (x_j - x_i)) + n_f2 (n_f2 . (x_j - x_i)) of edge slot s (slot
 * handling exactly as in fgc_vertex_update: an unused or out-of-range slot, the endpoint that is i itself and a missing
 * face add nothing):
 *   t_i += lambda * sum_s (u_s . d_i)   (slot order),      x_i = fma(t_i, d_i, x0_i)   per coordinate, x0 = the INPUT x.
 * The position is always rebuilt from the input position and the accumulated scalar, never by adding a step to the
 * previous iterate: in exact arithmetic the reference's rule, and a vertex stays within one rounding of its ray whatever
 * the iteration count.  x_out [nv,3]; t_out [nv] (may be NULL) receives t, the signed correction along the ray (in
 * units of |d|).  iters == 0: x_out = x bit for bit, t_out = 0.  ws: at least fgc_vertex_update_dir_workspace_floats(nv)
 * floats; x may alias neither x_out nor ws; e_map may be NULL when ne == 0.  Only enqueues: one launch per iteration, one
 * thread per vertex, ping-ponging between x_out and ws; allocates nothing. */
size_t fgc_vertex_update_dir_workspace_floats(int32_t nv);
int fgc_vertex_update_dir(const float* x, float* x_out, float* t_out, float* ws, size_t ws_floats, int32_t nv,
                          const float* normals, int32_t nf, const int32_t* e_map, int32_t ne, const int32_t* v_e_map,
                          int32_t max_edges, const float* dirs, int32_t n_dirs, int32_t iters, float lambda, void* stream);

/* 4:1 "average ignoring zero rows" pooling = custom_binary_tree_pooling(x, steps=2, 'avg_ignore_zeros')
 * (model.py:792-814): two rounds of pairwise means in which a row that is zero in every channel is replaced by its
 * partner first.  x [n, c] with n % 4 == 0 -> y [n/4, c]. */
int fgc_pool4_avg_iz(const float* x, int32_t n, int32_t c, float* y, void* stream);

/* Node centres of the finest level = first step of updateFacesCenter (train.py:1779-1787): barycentre of every face
 * of faces [n0,3] (int32, -1 corners read a zero vertex) -> fpos [n0,3]. */
int fgc_face_centers(const float* x, int32_t nv, const int32_t* faces, int32_t n0, float* fpos, void* stream);

/* Multi-scale vertex update = update_position_MS with updateFacesCenter (train.py:1668-1798), coarsening_steps = 2.
 * x [nv,3] positions; faces [n0,3] int32 in node order, -1 rows = fake nodes; v_faces [nv,k_v] finest-level node ids
 * of every vertex, -1 padded; normals[s] [n0 / 4^s, 3] for s = 0,1,2.  Coarse to fine, iters[0] iterations with the
 * level-2 nodes, iters[1] with level 1, iters[2] with level 0; in every iteration the node centres are recomputed
 * from the current positions (face barycentres, then two avg_ignore_zeros poolings) and
 *   x_v += (1 / #faces(v)) * sum_k n (n . (c - x_v)),  n, c of node floor(v_faces[v,k] / 4^s).
 * x_out [nv,3] receives the result; dx_out (may be NULL) [3][nv,3] the displacement of each stage in execution
 * order; scratch: at least 3*(nv*2 + n0 + n0/4 + n0/16) floats.  x may alias neither output. */
int fgc_vertex_update_ms(const float* x, float* x_out, int32_t nv, const int32_t* faces, int32_t n0,
                         const int32_t* v_faces, int32_t k_v, const float* normals0, const float* normals1,
                         const float* normals2, const int32_t* iters, float* dx_out, float* scratch,
                         size_t scratch_floats, void* stream);

/* Trajectory form of fgc_vertex_update_ms, for training through it: the same launches with the same arithmetic (the
 * result is bit-identical), every iteration writing a slot of its own.  traj [T+1][nv,3], T = iters[0] + iters[1] +
 * iters[2]: slot 0 receives x, slot t + 1 the positions after iteration t (slot T is fgc_vertex_update_ms's x_out; a
 * stage's dx is the difference of the slots at its ends).  scratch: at least 3*(n0 + n0/4 + n0/16) floats (the node
 * centres).  x may not lie in traj. */
int fgc_vertex_update_ms_traj(const float* x, int32_t nv, const int32_t* faces, int32_t n0, const int32_t* v_faces,
                              int32_t k_v, const float* normals0, const float* normals1, const float* normals2,
                              const int32_t* iters, float* traj, size_t traj_floats, float* scratch,
                              size_t scratch_floats, void* stream);

/* Adjoint of fgc_vertex_update_ms: given g_out = dL/d x_out [nv,3] and the trajectory fgc_vertex_update_ms_traj wrote,
 * g_x [nv,3] = dL/dx and g_n<s> [n0/4^s,3] = dL/d normals<s> (overwritten).  Per forward iteration at level s, with
 * a_v = g_v / #faces(v) and A_j, S_j the sums of a_v and of a_v x_v^T + x_v a_v^T over the slots (v,k) whose node is j:
 *   dL/dx_v = g_v - sum_k n_j (n_j . a_v) + (barycentre and pooling adjoints of dL/dc),  dL/dc_j = n_j (n_j . A_j),
 *   dL/dn_j += (A_j . n_j) c_j + (n_j . c_j) A_j - S_j n_j.
 * The centres are recomputed from the trajectory by the forward's kernels; the pooling adjoint makes the forward's
 * zero-row choices.  Two inverse tables, built once per mesh (int32, CSR):
 *   slot_ptr [n0+1], slot_vert: for every fine node f, the vertices v of the slots v_faces[v,k] == f, in (v, k) order
 *     (a slot table truncated to k_v slots keeps only the slots it has);
 *   inc_ptr [nv+1], inc_face: for every vertex, the faces that name it as a corner, once per corner, in (face, corner)
 *     order.
 * Every entry must lie in range (vertices < nv, nodes < n0).  traj_floats: the size of traj, at least (T+1)*3*nv.
 * workspace: at least
 * fgc_vertex_update_ms_bwd_workspace_floats(nv, n0) floats.  No atomics: the same bits from run to run.  A vertex
 * without faces passes its gradient straight through (it does not move).  g_out may not alias g_x. */
size_t fgc_vertex_update_ms_bwd_workspace_floats(int32_t nv, int32_t n0);
int fgc_vertex_update_ms_bwd(const float* traj, size_t traj_floats, int32_t nv, const int32_t* faces, int32_t n0, const int32_t* v_faces,
                             int32_t k_v, const float* normals0, const float* normals1, const float* normals2,
                             const int32_t* iters, const int32_t* slot_ptr, const int32_t* slot_vert,
                             const int32_t* inc_ptr, const int32_t* inc_face, const float* g_out, float* g_x,
                             float* g_n0, float* g_n1, float* g_n2, float* workspace, size_t workspace_floats,
                             void* stream);

/* The multi-scale vertex update along a per-vertex direction (a build extension: the reference constrains the
 * single-scale update only, update_position_with_depth) - fgc_vertex_update_ms with the step of every iteration
 * projected onto the direction d_v of its vertex, for the vertices of a depth scan, which may move along their viewing
 * rays only.  dirs [n_dirs,3] as in fgc_vertex_update_dir: row v when n_dirs == nv, the one row when n_dirs == 1, any
 * other n_dirs is FGC_EINVAL; d is used as given, nothing is normalised.  With delta_v = (1 / #faces(v)) sum_k n (n . (c -
 * x_v)) of fgc_vertex_update_ms (same slot handling, same centre launches per iteration), one iteration is
 *   t_v += delta_v . d_v,      x_v = fma(t_v, d_v, x0_v)   per coordinate, x0 = the INPUT x through all three stages:
 * in exact arithmetic x' = x + d (d . delta(x)).  t starts at 0 and accumulates across the stages; a vertex stays within
 * one rounding of its ray whatever the iteration counts.  The gain of a step is |d|^2: rows longer than 1 can diverge
 * (norms up to 2 reached 1e2 after 80 + 20 + 20 iterations on a 642-vertex sphere); unit rows, or shorter ones, are safe.
 * x_out [nv,3]; t_out [nv] (may be NULL) the signed step along d; dx_out (may be NULL) [3][nv,3] end minus start of each
 * stage, as in fgc_vertex_update_ms.  iters = {0,0,0}: x_out = x bit for bit, t_out = 0.  A vertex without faces does
 * not move.  scratch: at least fgc_vertex_update_ms_dir_scratch_floats(nv, n0) floats; x, x_out, t_out, dx_out and the
 * scratch are buffers of their own (no two may overlap).  Only enqueues (t is zeroed by an enqueued memset), allocates nothing. */
size_t fgc_vertex_update_ms_dir_scratch_floats(int32_t nv, int32_t n0);
int fgc_vertex_update_ms_dir(const float* x, float* x_out, int32_t nv, const int32_t* faces, int32_t n0,
                             const int32_t* v_faces, int32_t k_v, const float* normals0, const float* normals1,
                             const float* normals2, const int32_t* iters, const float* dirs, int32_t n_dirs, float* t_out,
                             float* dx_out, float* scratch, size_t scratch_floats, void* stream);

/* Trajectory form of fgc_vertex_update_ms_dir (the same launches, the same arithmetic: slot T is bit-identical to its
 * x_out): traj [T+1][nv,3], slot 0 = x, slot k + 1 = the positions after iteration k.  scratch: the size above serves (t
 * and the node centres, nv + 3*(n0 + n0/4 + n0/16) floats, are used).  x, traj, t_out (may be NULL) and the scratch are
 * buffers of their own. */
int fgc_vertex_update_ms_dir_traj(const float* x, int32_t nv, const int32_t* faces, int32_t n0, const int32_t* v_faces,
                                  int32_t k_v, const float* normals0, const float* normals1, const float* normals2,
                                  const int32_t* iters, const float* dirs, int32_t n_dirs, float* traj, size_t traj_floats,
                                  float* t_out, float* scratch, size_t scratch_floats, void* stream);

/* Adjoint of fgc_vertex_update_ms_dir on the trajectory fgc_vertex_update_ms_dir_traj wrote: fgc_vertex_update_ms_bwd
 * (same tables, same outputs, no atomics, the same bits from run to run) with the incoming gradient of every iteration
 * projected where it enters delta, gp_v = d_v (d_v . g_v):
 *   dL/dx_v = g_v - sum_k n_j (n_j . a_v) + (barycentre and pooling adjoints of dL/dc),   a_v = gp_v / #faces(v),
 * and A_j, S_j, dL/dc_j, dL/dn_j of fgc_vertex_update_ms_bwd on that a_v; the identity term keeps the unprojected g_v.
 * No gradient with respect to dirs.  workspace: at least fgc_vertex_update_ms_dir_bwd_workspace_floats(nv, n0) floats. */
size_t fgc_vertex_update_ms_dir_bwd_workspace_floats(int32_t nv, int32_t n0);
int fgc_vertex_update_ms_dir_bwd(const float* traj, size_t traj_floats, int32_t nv, const int32_t* faces, int32_t n0,
                                 const int32_t* v_faces, int32_t k_v, const float* normals0, const float* normals1,
                                 const float* normals2, const int32_t* iters, const float* dirs, int32_t n_dirs,
                                 const int32_t* slot_ptr, const int32_t* slot_vert, const int32_t* inc_ptr,
                                 const int32_t* inc_face, const float* g_out, float* g_x, float* g_n0, float* g_n1,
                                 float* g_n2, float* workspace, size_t workspace_floats, void* stream);

/* Point-set loss fullLoss (train.py:1373-1424) and its gradient.  p0 [np0,3] refined vertices, p1 [np1,3] ground-truth
 * vertices, i0 [ns0] rows of p0 and i1 [ns1] rows of p1 (repeats allowed):
 *   precision_i = min_j |p0[i0_i] - p1_j|,  completeness_i = min_j |p0_j - p1[i1_i]|,
 *   loss[0] = 1000 (mean(precision <= threshold ? precision : 0) + mean(completeness <= threshold ? completeness : 0)).
 * The nearest points come from fgc_nn_query.  g_p0 (may be NULL) [np0,3] receives dL/dp0 (dL/dloss = 1): a kept term
 * adds 1000/ns (p0_row - p1_nn) / d to its p0 row; terms sharing a row are summed in a fixed order (no atomics).
 * Two departures from TensorFlow's gradient: at d = 0 the term's gradient is 0 (TensorFlow: NaN), and an exact tie between
 * nearest points sends the whole gradient to the lowest index (tf.reduce_min splits it).  A sample index out of range
 * makes the loss NaN.  workspace (device, 256-byte aligned) >= fgc_point_loss_workspace_bytes(np0, np1, ns0, ns1).
 * ns0 + ns1 <= FGC_POINT_LOSS_MAX_SAMPLES: the row reduction runs in one workgroup and costs O((ns0 + ns1)^2) compares
 * (the reference samples 500 + 500). */
#define FGC_POINT_LOSS_MAX_SAMPLES 16384
size_t fgc_point_loss_workspace_bytes(int32_t np0, int32_t np1, int32_t ns0, int32_t ns1);
int fgc_point_loss(const float* p0, int32_t np0, const float* p1, int32_t np1, const int32_t* i0, int32_t ns0,
                   const int32_t* i1, int32_t ns1, float threshold, float* loss, float* g_p0, void* workspace,
                   size_t workspace_bytes, void* stream);

/* Dense face-normal loss of trainDoubleLossNet: faceNormalsLoss (train.py:1272-1294) over ALL n rows, against the
 * ground truth rotated on the fly (train.py:1019-1021).  fn [n,3]: head 0, normalised; gt [n,3]: the UNROTATED ground
 * truth; R: device pointer to 9 floats (row-major, applied as fgc_rotate_rows does) or NULL (identity).  A row whose
 * rotated ground truth has an L1 norm <= 1e-3 is a fake node and does not count.  Per row the same arithmetic as
 * fgc_rotate_rows + fgc_angular_loss_fwd / _bwd (they agree row for row; the loss differs only in the order of the sum).
 *   fwd: one partial {sum of angles, real rows} per 256 rows into scratch, then loss_out [2] = {loss in degrees, real
 *     rows} (no real row: 0 / 0).  add / total (both NULL or both given, device scalars): total[0] = add[0] + loss[0]
 *     (the step's sum of the point-set and the normal loss stays on the device).  Two launches.
 *   bwd: g_fn [n,3] is ADDED TO (not overwritten): every real row strictly inside the clip gets
 *     dloss k (R gt_r), k = -(180/pi) / sqrt(1 - dt^2) / (real rows); the real-row count comes from the partials the
 *     forward left in scratch.  One launch, one writer per row, no atomics.
 * scratch: at least fgc_dense_normals_loss_scratch_floats(n) floats, kept between the forward and the backward. */
size_t fgc_dense_normals_loss_scratch_floats(int32_t n);
int fgc_dense_normals_loss_fwd(const float* fn, const float* gt, const float* R, int32_t n, float* loss_out,
                               const float* add, float* total, float* scratch, size_t scratch_floats, void* stream);
int fgc_dense_normals_loss_bwd(const float* fn, const float* gt, const float* R, int32_t n, const float* scratch,
                               size_t scratch_floats, float dloss, float* g_fn, void* stream);

/* Nearest neighbour over point sets: the distance scan of hausdorffOverSampled (utils.py:816-1006) and of exact
 * point-set distances.  For every query point q[i] (float32 [nq,3]) the nearest point of p (float32 [np,3]) by squared
 * Euclidean distance, computed in fp32 in the reference's order (dx*dx + dy*dy) + dz*dz with every operation rounded
 * (no fused multiply-add): dist[i] = its distance (the correctly rounded fp32 sqrt of that value), idx[i] = its row.
 * Exact (brute force) and deterministic: equal squared distances resolve to the LOWEST index, and the result does not
 * depend on how the launch splits the work.  Candidates whose squared distance is NaN or +inf are never chosen.
 * Optional masks (both NULL, or both given), int32 [nq] / [np]: packed cell coordinates (i << 20) | (j << 10) | k with
 * 0 <= i, j, k < 512, or -1 for "in no cell".  Then candidate j counts for query i only if p_cell[j] lies in one of the
 * 2x2x2 cells (i..i+1, j..j+1, k..k+1) of q_cell[i] (the reference's partition: 5^3 query cells, 6^3 candidate cells).
 * A query with no candidate gets dist = +inf and idx = -1, and so does a query whose own cell is -1.
 * workspace (device, 8-byte aligned) >= fgc_nn_workspace_bytes(nq, np); two launches and a memset on `stream`. */
size_t fgc_nn_workspace_bytes(int32_t nq, int32_t np);
int fgc_nn_query(const float* q, int32_t nq, const float* p, int32_t np, const int32_t* q_cell, const int32_t* p_cell,
                 float* dist, int32_t* idx, void* workspace, size_t workspace_bytes, void* stream);

/* Bilateral normal filter over a list of triangles (utils.bilateralFilter / utils.FND, utils.py:2344-2496), all
 * P = S x R parameter pairs in one pass over the candidates.  For n faces with centres c [n,3], normals nrm [n,3], areas
 * a [n] (float32, device):
 *   out[i, 3p .. 3p+2] = normalize( sum over j in window(i) of a_j exp(-|c_i - c_j|^2 / (2 sigma_s^2))
 *                                                                 exp(-|n_i - n_j|^2 / (2 sigma_r^2)) n_j ),
 * p = s * R + r (sigma_s-major), out [n, 3 S R]; sigma_r = -1 means "no range term" (that factor is 1); normalize is
 * x * (1 / (|x| + 1e-8)) applied twice (utils.normalize), so a zero sum stays zero.  sigma_s [S], sigma_r [R]: HOST arrays.
 * The cells are an input: the grid has sx x sy x sz cells (1 .. FGC_BILATERAL_MAX_SLICES per axis), flattened as
 * (i * sy + j) * sz + k; cell_order [n] (device) is a permutation of the faces, those that lie in a cell first, ordered by
 * flattened cell, then the faces in no cell; cell_ptr [sx sy sz + 1] (device) is the range table over cell_order
 * (cell_ptr[cells] = number of faces in a cell).  window(i) = the faces of the cells that differ from face i's cell by at
 * most 1 on every axis, clipped at the grid's edge, face i included.  A face in no cell is in nobody's window and gets a
 * zero row.  Results are written in the caller's face order.
 * fp32 throughout, exp through the hardware exp2 with a pre-scaled argument.  Deterministic: every row's sum has one fixed
 * order (no floating-point atomics), and a pair's result does not depend on which other pairs the call computes.
 * Entries of cell_order outside [0, n) and ranges of cell_ptr outside [0, n] are ignored, never dereferenced.
 * workspace (device, 16-byte aligned) >= fgc_bilateral_workspace_bytes(n, sx, sy, sz) (0 for arguments the filter refuses;
 * the size also covers fgc_bilateral_filter_guided).
 * A memset, two small launches, then one launch per 4 x 3 block of (sigma_s, sigma_r) on `stream`. */
#define FGC_BILATERAL_MAX_SLICES 64
size_t fgc_bilateral_workspace_bytes(int32_t n, int32_t sx, int32_t sy, int32_t sz);
int fgc_bilateral_filter(const float* centres, const float* normals, const float* areas, int32_t n,
                         const int32_t* cell_order, const int32_t* cell_ptr, int32_t sx, int32_t sy, int32_t sz,
                         const float* sigma_s, int32_t S, const float* sigma_r, int32_t R, float* out, void* workspace,
                         size_t workspace_bytes, void* stream);

/* Guided normal filtering (BUILD EXTENSION - the reference stops at the bilateral filter; Zhang, Deng, Zhang, Bouaziz, Liu:
 * "Guided mesh normal filtering", 2015): the range term of the filter reads a guidance normal G instead of the noisy normal,
 * and G_i is the area-weighted mean normal of the most consistent patch among the patches that contain face i.
 * For n faces with unit normals N [n,3] and areas A [n] (float32, device):
 *   ring [n, ld] (int32, device): zero-based, -1 padded; slot 0 is the face itself, then the faces that share at least one
 *     vertex with it, each once (utils.face_rings: the row of getFacesLargeAdj with repeats dropped); ld a multiple of 4,
 *     4 <= ld <= FGC_GUIDED_MAX_RING, rows 16-byte aligned.  P(k) = the faces of ring[k].
 *   fe [n,3] (int32, device): the face across each edge of a face, -1 at a border (utils.face_edge_neighbours).
 *     E(k) = the edges whose two faces both lie in P(k), each once: the pairs (a, t) with a in P(k), fe[a, t] in P(k) and
 *     a < fe[a, t].
 *   Phi(k) = max over a, b in P(k) of |N_a - N_b|;  phi(e) = |N_a - N_b| for e = (a, b) in E(k)
 *   R(k)   = max_e phi(e) / (1e-9 + sum_e phi(e))  (0 when E(k) is empty);   H(k) = Phi(k) R(k)
 *   M(k)   = sum over a in P(k) of A_a N_a, in slot order
 *   pick(i)= the face k of ring[i] with the smallest H(k), the first such slot on a tie;  G_i = normalize(M(pick(i)))
 *     (utils.normalize: x * (1 / (|x| + 1e-8)) twice; a zero sum stays zero)
 * fgc_guided_normals writes guide_out [n,3] = G, and, where the pointers are not NULL, pick_out [n] (int32, -1 for a row
 * without a valid slot) and h_out [n] = H.  Two launches on `stream`: gd_patch_kernel ({M, H} per face into the workspace,
 * one row of 16 lanes per face) and gd_pick_kernel.  workspace (device, 16-byte aligned) >= fgc_guided_workspace_bytes(n, ld)
 * (0 for arguments the call refuses); after the call it holds one float4 (M_x, M_y, M_z, H) per face.
 * fgc_bilateral_filter_guided is fgc_bilateral_filter with exp(-|G_i - G_j|^2 / (2 sigma_r^2)) as its range term, guide
 * [n,3] (float32, device) given by the caller; window, order of the sum, sigma_r = -1, the handling of indices and the
 * workspace (fgc_bilateral_workspace_bytes) are those of fgc_bilateral_filter.
 * fp32 throughout, deterministic (no floating-point atomics); entries of ring outside [0, n) are skipped and entries of fe
 * are only compared, so no index outside [0, n) is ever dereferenced. */
#define FGC_GUIDED_MAX_RING 64
size_t fgc_guided_workspace_bytes(int32_t n, int32_t ld);
int fgc_guided_normals(const float* normals, const float* areas, int32_t n, const int32_t* ring, int32_t ld, const int32_t* fe,
                       float* guide_out, int32_t* pick_out, float* h_out, void* workspace, size_t workspace_bytes,
                       void* stream);
int fgc_bilateral_filter_guided(const float* centres, const float* normals, const float* areas, int32_t n,
                                const int32_t* cell_order, const int32_t* cell_ptr, int32_t sx, int32_t sy, int32_t sz,
                                const float* sigma_s, int32_t S, const float* sigma_r, int32_t R, const float* guide,
                                float* out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Noise synthesis: training from clean meshes (BUILD EXTENSION - the reference trains on noisy files prepared on the host)
 * ---------------------------------------------------------------------------------- */

/* Per step, the vertices of a clean mesh are displaced by a counter-based Gaussian draw and the six input channels of
 * every node row are rebuilt from the displaced vertices.  Definitions:
 *   Random numbers: Philox4x32-10, multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85,
 *     counter = (vertex index, step & 0xffffffff, step >> 32, stream_id), key = (seed & 0xffffffff, seed >> 32); step and
 *     seed are 64-bit, stream_id is the caller's 32-bit id (training 0, validation mesh i 1 + i).
 *   Gaussians: u_k = ((x_k >> 8) + 0.5) 2^-24 (never 0 or 1); r0 = sqrt(-2 ln u0), z0 = r0 cos(2 pi u1),
 *     z1 = r0 sin(2 pi u1); z2, z3 from (u2, u3) in the same way.  u_k needs 25 bits, so it is exact in fp32 only below
 *     1/2; above, 1 - u_k is exact and the kernel evaluates ln u as log1pf(-(1 - u)) and sin / cos of the angle
 *     -2 pi (1 - u); sin / cos come from the accurate sinpif / cospif on the exact 2 u (or 2 (1 - u)), not from sinf / cosf
 *     on an angle rounded to fp32: every function sees an exact argument (csrc/fgc_synth.h says what is lost otherwise).
 *   Displacement: vnormals == NULL: v' = v + d sigma z3 with d = (z0, z1, z2) / |(z0, z1, z2)|; otherwise
 *     v' = v + vnormals[i] sigma z3 (unit vertex normals of the clean mesh, [nv,3]).  sigma = 0 gives v' = v bit for bit.
 *   Features: x[i] = [n | centre] of face (a, b, c) = faces_rows[i] on the vertices, in fgc_face_features's arithmetic -
 *     cross product with separately rounded multiplies and subtracts, normalised twice with 1e-8 added to the norm, the
 *     bounding-box diagonal of the vertices in double from the fp32 extents then rounded to fp32, centre =
 *     ((q0 + q1) + q2) / 3 with q = p / diag - so bit-identical to that host routine; a row with a negative (or
 *     out-of-range) vertex id is a fake node and gets six zeros.
 * Control words ctl (DEVICE, 3 x uint32, read by the kernels - a replayed hipGraph draws new noise without re-capture):
 *   ctl[0], ctl[1] = step low / high; ctl[2] = 0: OFF, the launches read and write nothing (v_out, x and scratch stay as
 *   they are); otherwise bit 31 is the on flag and bits 0..30 the float bits of sigma >= 0 (FGC_SYNTH_ON | bits).
 * scratch (device floats) >= fgc_synth_scratch_floats(nv): fgc_synth_noise leaves the per-workgroup bounding boxes of
 * v_out there; fgc_face_features_rows(have_bbox = 1) reads them (same nv, same scratch, right behind it on the stream),
 * have_bbox = 0 computes them from v with one more launch.  ctl may be NULL for fgc_face_features_rows (always on).
 * Enqueue-only, nothing allocated: fgc_synth_noise is one launch, fgc_face_features_rows one (have_bbox) or two. */
#define FGC_SYNTH_ON 0x80000000u
size_t fgc_synth_scratch_floats(int32_t nv);
int fgc_synth_noise(const float* v, const float* vnormals, int32_t nv, const uint32_t* ctl, uint64_t seed,
                    uint32_t stream_id, float* v_out, float* scratch, size_t scratch_floats, void* stream);
int fgc_face_features_rows(const float* v, int32_t nv, const int32_t* faces_rows, int32_t n, const uint32_t* ctl,
                           int32_t have_bbox, float* x, float* scratch, size_t scratch_floats, void* stream);
/* The raw generator of fgc_synth_noise, for known-answer tests: out [n,4] uint32 (device, 16-byte aligned),
 * out[i] = Philox4x32-10 of counter (first + i mod 2^32, step & 0xffffffff, step >> 32, stream_id) and key seed.  One launch. */
int fgc_philox_words(uint32_t first, int32_t n, uint64_t step, uint64_t seed, uint32_t stream_id, uint32_t* out, void* stream);

/* Low-frequency noise (BUILD EXTENSION; the reference's utils.addLFGaussianNoise, utils.py:2310-2319, is an unfinished stub
 * of the same idea): fgc_synth_noise plus a smooth field, a sum of K = n_bumps Gaussian bumps centred on randomly chosen
 * CLEAN vertices, evaluated with Euclidean distances on the clean mesh; every vertex moves by the field along its clean
 * unit vertex normal.
 *   bump k in [0, K): (x0, x1, x2, x3) = Philox4x32-10(counter = (k, step & 0xffffffff, step >> 32, stream_id | 0x80000000),
 *                     key = seed);  c_k = (x0 * nv) >> 32 (the centre is clean vertex c_k; x1 is reserved);
 *                     a_k = A z, z the first Gaussian of the pair (x2, x3) as defined above (z0 of u0 = x2, u1 = x3)
 *   field             s_i = sum_k a_k exp(-|v_i - v_{c_k}|^2 / (2 w^2))           (fp32, clean vertices)
 *   output            v_out_i = white_i + vnormals_i s_i
 *   white_i is what fgc_synth_noise(v, white_normals, ...) writes for the same (ctl, seed, stream_id): with sigma 0 the
 *   clean vertex.  The top bit of the stream word separates the bump counters from the per-vertex ones, so stream_id must
 *   be below 2^31.  A >= 0: the amplitude, w > 0: the width, both in mesh units.  Centres are uniform over the VERTICES (not
 *   over the area), and the distance is Euclidean, not geodesic: a bump reaches through a sheet thinner than w.
 * lf_ctl (DEVICE, 4 x uint32, read by the kernels like ctl): {FGC_SYNTH_ON | float bits of A, float bits of w, 0, 0};
 *   lf_ctl[0] = 0: bumps off - v_out and the scratch's bounding boxes get the bits fgc_synth_noise leaves.  ctl[2] = 0
 *   switches everything off, as for fgc_synth_noise.
 * vnormals [nv,3] is required (the bumps always go along it); white_normals is fgc_synth_noise's vnormals: NULL = the white
 *   draw takes a random direction.
 * Arithmetic: d2 = fma(dz, dz, fma(dy, dy, dx dx)); the exponential is the hardware exp2 of d2 * (-log2 e / (2 w w)) (about
 *   1 ulp, on an argument rounded twice: the relative error of a term grows with its exponent); the terms are added in bump
 *   order within a slice of K and the slices in slice order; the slicing depends on (nv, K) alone, and there are no
 *   floating-point atomics: the same call gives the same bits, eager or replayed from a hipGraph.
 * scratch (device floats, 16-byte aligned) >= fgc_synth_lf_scratch_floats(nv, n_bumps) (0 for arguments out of range): its
 *   first fgc_synth_scratch_floats(nv) floats are the bounding boxes of the final v_out, as fgc_synth_noise leaves them for
 *   fgc_face_features_rows / fgc_point_sets_prepare(have_bbox = 1); behind them, at the next multiple of 4 floats, the
 *   bump table [n_bumps, 4] = {centre x, y, z, a_k} as the last ON call left it, then the slices' partial sums and one
 *   arrival counter per vertex block.
 * Two launches, enqueue-only, nothing allocated: the table (one thread per bump), then field + displacement (one vertex
 *   per lane, the table wave-uniform through scalar loads; nv x K pairs, no spatial culling).  A NULL among v, vnormals, ctl,
 *   lf_ctl, v_out, scratch, nv <= 0, v_out == v, n_bumps outside 1 ... FGC_SYNTH_LF_MAX_BUMPS, stream_id >= 2^31, a scratch
 *   that is misaligned or too small: FGC_EINVAL, nothing launched. */
#define FGC_SYNTH_LF_MAX_BUMPS (1 << 20)
size_t fgc_synth_lf_scratch_floats(int32_t nv, int32_t n_bumps);
int fgc_synth_noise_lf(const float* v, const float* vnormals, const float* white_normals, int32_t nv, const uint32_t* ctl,
                       const uint32_t* lf_ctl, int32_t n_bumps, uint64_t seed, uint32_t stream_id, float* v_out,
                       float* scratch, size_t scratch_floats, void* stream);

/* Depth-sensor noise (BUILD EXTENSION): fgc_synth_noise along a table of viewing rays, with the two properties of a
 * triangulating sensor (structured light, stereo) - the error grows with the range, and the depth is quantised in
 * disparity: the sensor reports r = 1 / (k q) for an integer k, so the depth step grows with r^2.  A perspective view only:
 * a camera c and one unit ray per vertex, dirs [nv,3], taken as given (utils.view_rays makes normalize(v - c)).
 * For clean vertex i, d_i = dirs[i], everything in fp32, one rounding per operation (no contraction):
 *   w     = v_i - c
 *   r_i   = sqrtf(fma(w_z, w_z, fma(w_y, w_y, w_x w_x)))
 *   rho_i = r_i / r_ref                                    (IEEE division)
 *   s_i   = sigma (power 0);  sigma * rho_i (power 1);  (sigma * rho_i) * rho_i (power 2)
 *   len_i = s_i * z3_i        z3: the Gaussian fgc_synth_noise draws - the same Philox counter (i, step, stream_id), key
 *                             and pair of words, so the same number
 *   q = 0 (no quantisation):  v'_i = v_i + d_i * len_i, fgc_synth_noise's expression with s_i in the place of sigma: with
 *     power 0 the output is BIT FOR BIT what fgc_synth_noise(v, dirs, ...) writes; sigma = 0 gives v' = v bit for bit.
 *   q > 0:  rt = r_i + len_i; a sample with rt <= 0 (the noise carried it through the sensor) takes rt = r_i;
 *           k = rintf(1 / (rt * q))  (two IEEE operations, ties to even), clamped to [1, 2^24];
 *           r_q = 1 / (k * q);  len'_i = r_q - r_i;  v'_i = v_i + d_i * len'_i.
 *     sigma = 0 with q > 0 quantises the clean range (terraces alone).
 *   power is an integer (there is no powf); sigma is the standard deviation AT THE REFERENCE RANGE r_ref; q is in 1 / length:
 *   the depth step at range r is r^2 q.  utils.sensor_model derives r_ref and q from a mesh, a camera and a step in mean
 *   edge lengths.
 * ctl: fgc_synth_noise's {step low, step high, sigma word}; ctl[2] = 0: off, nothing read or written.
 * sensor_ctl (DEVICE, 4 x uint32, read by the kernel like ctl - a replayed hipGraph can change level, power and step without
 *   a new capture): {FGC_SYNTH_ON | power, float bits of r_ref, float bits of q, 0}.  THIS BUILD'S CHOICE for words out of
 *   range - sensor_ctl[0] without the on flag (0 included), power > 2, r_ref not a positive normal finite float, q neither
 *   zero nor a positive normal finite float: the model is OFF and the launch writes the bits of
 *   fgc_synth_noise(v, dirs, ...), plain noise along the rays; such words never give a non-finite vertex.  (The host cannot
 *   refuse words it does not see; ops.sensor_words refuses the same values before they reach the device.)
 * camera: a HOST pointer to three finite floats, read during the call and passed to the kernel BY VALUE: it is fixed per
 *   bound mesh, and a captured launch keeps the values it was recorded with.
 * scratch (device floats) >= fgc_synth_scratch_floats(nv): the per-workgroup bounding boxes of v_out, exactly as
 *   fgc_synth_noise leaves them: fgc_face_features_rows(have_bbox = 1) and fgc_point_sets_prepare(have_bbox = 1) follow it
 *   unchanged.
 * One launch of fgc_synth_noise's shape (256 threads, one vertex per thread, grid-stride above 1024 workgroups), accurate
 *   division and sqrtf, no atomics: the same bits eager and replayed.  Enqueue-only, nothing allocated.  A NULL among v,
 *   dirs, ctl, sensor_ctl, camera, v_out, scratch, nv <= 0, v_out == v, a non-finite camera or a scratch below
 *   fgc_synth_scratch_floats(nv): FGC_EINVAL, nothing launched. */
int fgc_synth_noise_sensor(const float* v, const float* dirs, int32_t nv, const uint32_t* ctl, const uint32_t* sensor_ctl,
                           const float* camera, uint64_t seed, uint32_t stream_id, float* v_out, float* scratch,
                           size_t scratch_floats, void* stream);

/* The two point sets of the point-set loss (fgc_point_loss) from displaced vertices: what the host does with
 * normalizePointSets (utils.py:2077-2104) and two fgc_rotate_rows, in ONE launch per step.
 *   v [nv,3]: the displaced vertices (fgc_synth_noise's v_out); gt [ngt,3]: the ground-truth vertices in the same raw
 *   units; gt_box (device, 6 floats): {min xyz, max xyz} of gt, made once per mesh; R: device pointer to 9 floats
 *   (row-major, applied as fgc_rotate_rows does) or NULL (identity).
 *   scratch (device floats) >= fgc_synth_scratch_floats(nv): with have_bbox = 1 it holds the per-workgroup bounding
 *   boxes fgc_synth_noise left for v (same nv, same scratch, right behind it on the stream - fgc_face_features_rows in
 *   between leaves them alone); have_bbox = 0 computes them from v first, one more launch.
 * Arithmetic: the bounding box of the UNION = the boxes of v reduced together with gt_box (min / max are exact: any
 *   order); the diagonal in double from the fp32 extents, rounded to fp32; every coordinate is DIVIDED by it in IEEE fp32
 *   (not multiplied by a reciprocal: numpy divides, and the two differ in the last bit); then out = R q with
 *   out_i = fma(R_i2, q_2, fma(R_i1, q_1, R_i0 q_0)), the association of fgc_rotate_rows.  So v_out / gt_out are
 *   bit-identical to normalizePointSets(v, gt) followed by fgc_rotate_rows (R given) or to normalizePointSets alone
 *   (R == NULL).  A union box of zero extent divides by zero, as the host routine does.
 * There is NO control word: the launch always runs, on what v and scratch hold (a step whose noise words are zero
 *   normalises what the last ON step left).  v_out [nv,3], gt_out [ngt,3]: buffers of their own (not v, not gt).
 * One thread per 3-vector of the two sets; every workgroup reads the boxes (at most 1024 x 24 bytes + gt_box), R and its
 *   256 vectors.  Enqueue-only, nothing allocated, no atomics: one launch (have_bbox) or two.  A NULL among v, gt, gt_box,
 *   v_out, gt_out, scratch, nv <= 0, ngt <= 0 or a scratch below fgc_synth_scratch_floats(nv): FGC_EINVAL, nothing launched. */
int fgc_point_sets_prepare(const float* v, int32_t nv, const float* gt, int32_t ngt, const float* gt_box, const float* R,
                           int32_t have_bbox, float* v_out, float* gt_out, float* scratch, size_t scratch_floats,
                           void* stream);

/* ------------------------------------------------------------------------------------
 * Ray casting: virtual depth scans (BUILD EXTENSION - the reference has no such primitive; its scans are downloads)
 * ---------------------------------------------------------------------------------- */

/* For every ray q in [0, nq) the first triangle of a list that it meets, brute force over rays x triangles (no spatial
 * culling: the cost grows with nq x nf).  Made for preparation time - which vertices a camera sees (utils.visible_vertices),
 * a depth image (utils.depth_image) - not for a training step.
 *   Ray q: o_q + t d_q.  o_q = row q of origins [n_origins,3], the one row when n_origins == 1 (a camera); d_q = row q of
 *     dirs [nq,3], used as given and never normalised: t is in units of |d_q|.
 *   Triangle f = (a, b, c) = faces[f] on verts [nv,3] takes part only if all three ids lie in [0, nv); other rows are
 *     skipped and never dereferenced.
 *   Intersection (Moeller-Trumbore, two-sided), with x . y = fma(x_z, y_z, fma(x_y, y_y, x_x y_x)) and
 *     (x x y)_i = fma(x_j, y_k, -(x_k y_j)) for (i, j, k) a cyclic shift of (x, y, z):
 *       e1 = b - a, e2 = c - a, p = d x e2, det = e1 . p            (det == 0: the triangle is skipped)
 *       s = o - a, u = (s . p) / det, qv = s x e1, v = (d . qv) / det, t = (e2 . qv) / det
 *     a hit iff u >= 0, v >= 0, u + v <= 1, t > t_min and t is finite.  fp32 throughout, IEEE divisions, no contraction:
 *     every fused operation is one of the fma above.  (det == 0 makes t an infinity or a NaN, which is no hit.)
 *   Result: the smallest t over the hits, among equal t the smallest face index; t_out [nq], face_out [nq], bary_out [nq,2]
 *     = (u, v) of the winner (may be NULL).  A miss: t_out = +inf, face_out = -1, bary_out = (0, 0).
 * The minimum over (t, face) is exact - each workgroup's result goes into a 64-bit integer atomic min on
 *   (float bits of t) << 32 | face, and t > t_min >= 0 orders like its bits - so the result does not depend on how the launch
 *   splits rays and triangles, and is the same bits eager or replayed from a hipGraph.  No floating-point atomics.
 * A call with n_origins == 1 gives the bits of the same call with that row repeated nq times (the same kernel).
 * workspace (device, 16-byte aligned) >= fgc_ray_cast_workspace_bytes(nf, nq) (0 for arguments out of range): one record of
 *   three float4 per triangle, (a, 0), (e1, 0), (e2, 0), nf rounded up to a multiple of 4 (an invalid row and the padding
 *   are zero records: det = 0), then one 64-bit key per ray.
 * Three launches, enqueue-only, nothing allocated: the records (and the keys' initial value), rays x triangles (64 rays per
 *   workgroup, the records wave-uniform through scalar loads, the triangle list split over blockIdx.y when the rays alone
 *   do not fill the device), keys -> outputs.  A NULL among verts, faces, origins, dirs, t_out, face_out, workspace;
 *   nv, nf or nq <= 0; nf > FGC_RAY_CAST_MAX_FACES; n_origins neither 1 nor nq; t_min negative, infinite or a NaN; a
 *   workspace that is misaligned or too small: FGC_EINVAL, nothing launched. */
#define FGC_RAY_CAST_MAX_FACES (1 << 30)
size_t fgc_ray_cast_workspace_bytes(int32_t nf, int32_t nq);
int fgc_ray_cast(const float* verts, int32_t nv, const int32_t* faces, int32_t nf, const float* origins, int32_t n_origins,
                 const float* dirs, int32_t nq, float t_min, float* t_out, int32_t* face_out, float* bary_out,
                 void* workspace, size_t workspace_bytes, void* stream);

/* The same cast through a bounding-box tree, at a cost that does not grow with nq x nf.  Two steps: fgc_ray_tree_build once
 * per mesh, fgc_ray_cast_tree once per set of rays (any number of views share a build).
 *
 * THE TREE is implicit: no topology is stored, it is defined by an order of the triangles alone.
 *   order [nf] int32: a permutation of 0 .. nf-1, device memory.  Nothing about it is checked on the host; on the device an
 *     entry outside [0, nf) yields a zero record.  ANY permutation gives a valid tree with the same results; only the speed
 *     depends on it (ops.ray_tree sorts the faces along a Morton curve of their centroids).
 *   Records: record j = the record fgc_ray_cast makes of face order[j] - (a, 0), (e1, 0), (e2, 0), 48 bytes, a zero record
 *     for a row with a vertex id outside [0, nv) - with face_of[j] = order[j] beside it; nf is rounded up to whole chunks of
 *     4 with zero records.
 *   Leaves: leaf i = the chunk of records 4i .. 4i + 3.  Its box is the exact min / max over the ORIGINAL three vertices
 *     verts[a], verts[b], verts[c] (not a + e1) of those of its faces that are valid and whose nine coordinates are finite; a
 *     face with a bad id or a non-finite coordinate contributes nothing (fgc_ray_cast never reports a hit on a NaN either),
 *     and a leaf without such a face has the empty box lo = +inf, hi = -inf.
 *   Nodes: a node is 8 children, stored as their 8 boxes of 6 floats (lo.xyz, hi.xyz): 48 dwords, three 16-dword scalar
 *     loads, the size of a chunk of records.  n[0] = leaves, n[L] = ceil(n[L-1] / 8); node k of level L >= 1 holds the boxes
 *     of children 8k .. 8k + 7 of level L - 1 (leaves for L = 1), a missing child is the empty box; the level whose n is 1
 *     is the root (10 levels for 2^30 faces).  A box above the leaves is the union of its children, min / max again: exact.
 *   tree (device, 16-byte aligned) >= fgc_ray_tree_bytes(nf) bytes (0 for nf <= 0 or nf > FGC_RAY_CAST_MAX_FACES; it never
 *     decreases with nf): the records, face_of, then the nodes level by level from the bottom.  It holds no pointer and no
 *     index that is used to address memory.
 *   fgc_ray_tree_build: one launch for the leaves (one thread per box: records, face_of, box) and one per level above (one
 *     thread per box).  Enqueue-only, capturable, nothing allocated.  A NULL among verts, faces, order, tree; nv or nf <= 0;
 *     nf > FGC_RAY_CAST_MAX_FACES; a tree that is misaligned or too small: FGC_EINVAL, nothing launched.
 *
 * THE CAST.  Arguments and outputs mean what they mean in fgc_ray_cast (nf is the nf of the build); a miss is
 *   (+inf, -1, (0, 0)), the barycentrics are those rc_uvt gave for the winner.  The per-pair arithmetic is the ONE function
 *   fgc_ray_cast runs, on the same record, so a pair tested by both gives the same bits; the tree tests a subset of the pairs.
 *   Hence on every ray the tree's (t, face) is never smaller in key order than fgc_ray_cast's, and it is equal wherever the
 *   boxes do not cull the winner.  fp32 Moeller-Trumbore is not watertight: it can report a hit on a grazed triangle whose box
 *   the exact ray misses, and the tree may cull that one.
 *   Traversal by packet: a wave holds 64 rays, one per lane; its stack of (node, ballot) entries is wave-uniform, the boxes of
 *   a node and the records of a leaf arrive through scalar loads.  A lane takes part in a node only if its own ray met that
 *   node and every node above it; it tests the four records of a leaf only if its ray meets the leaf's box in
 *   [t_min, best_t] with the best_t it has at that moment; it keeps the smallest (t, face_of) in FULL key order
 *   (t < best_t, or t == best_t and face < best_face: records are not in rising face order).  Children are visited in index
 *   order.  So the leaves a lane tests, and the best_t it tests each with, are those of its ray walking the tree alone: a
 *   ray's result is a function of the tree and that ray - not of its neighbours in the wave, the launch geometry, the order
 *   of the rays, eager or replayed.  A lane beyond nq takes part in no ballot.
 *   THE SLAB TEST of a lane's ray against a box (lo, hi), inv = (1 / d_x, 1 / d_y, 1 / d_z) in IEEE (a zero component gives
 *   an infinity): per axis t1 = (lo - o) inv, t2 = (hi - o) inv (one subtraction, one multiplication), tn = t1 and tf = t2
 *   if inv >= 0, swapped otherwise; near = max(tn_x, tn_y, tn_z), far = min(tf_x, tf_y, tf_z) with min / max that return the
 *   operand that is no NaN; near' = near - (|near| 2^-21 + 2^-125), far' = far + (|far| 2^-21 + 2^-125).  The lane meets the
 *   box iff near' <= far', far' >= t_min and near' <= best_t, all non-strict (an equal t on a lower face index behind a box
 *   entered at exactly best_t is still found).
 *   Why it never rejects a box the exact ray passes through (for 1 / d finite or d == 0, and t within the range of fp32):
 *   the exact parameters of the two planes are (lo - o) / d and (hi - o) / d.  The subtraction, the reciprocal and the
 *   product each round once, so a computed t is the exact one times (1 + e)^3, |e| <= 2^-24: off by less than 2 units in
 *   the last place and never of the wrong sign; a product that underflows is off by less than 2^-126.  near' and far' move
 *   each end outward by 4 units and 2^-125, more than that error, and rounding is monotonic, so near' <= exact near and
 *   far' >= exact far: if the exact interval is not empty and meets [t_min, best_t], the computed one does.  Which of t1, t2
 *   is the near one is decided by the sign of inv, not by comparing them, so with d == 0 on an axis: an origin strictly
 *   inside the slab gives tn = -inf, tf = +inf (no constraint); outside it, tn = +inf or tf = -inf (rejected, rightly: the
 *   ray never enters); ON a plane, 0 x inf = NaN on that side, which max / min drop: the plane does not constrain, the ray
 *   counts as inside.  An empty box gives near = +inf or far = -inf on every axis and is never met; so is any box for a ray
 *   with a NaN, which can hit nothing.  (Ize, "Robust BVH Ray Traversal", JCGT 2013, is the usual statement of this test.)
 *   NO LOOP ENDS ON DEVICE DATA: each node is pushed at most once, so the walk pops at most (number of nodes) times, a count
 *   made on the host from nf; the stack holds at most 7 entries per level + 1; every popped id is bounded before it addresses
 *   anything.  A corrupt tree gives wrong answers, not a hang and no access outside the buffer.
 *   No per-call workspace, no key buffer, no atomics: each ray is owned by one lane.  One launch, enqueue-only, capturable.
 *   A NULL among tree, origins, dirs, t_out, face_out; nf or nq <= 0; nf > FGC_RAY_CAST_MAX_FACES; n_origins neither 1 nor nq;
 *   t_min negative, infinite or a NaN; a tree that is misaligned or below fgc_ray_tree_bytes(nf): FGC_EINVAL, nothing
 *   launched. */
size_t fgc_ray_tree_bytes(int32_t nf);
int fgc_ray_tree_build(const float* verts, int32_t nv, const int32_t* faces, int32_t nf, const int32_t* order, void* tree,
                       size_t tree_bytes, void* stream);
int fgc_ray_cast_tree(const void* tree, size_t tree_bytes, int32_t nf, const float* origins, int32_t n_origins,
                      const float* dirs, int32_t nq, float t_min, float* t_out, int32_t* face_out, float* bary_out,
                      void* stream);

/* Closest point on the mesh of a tree, for every point q in [0, nq): the walk of fgc_ray_cast_tree with a distance bound in
 * place of the slab test.  tree, tree_bytes, nf: those of fgc_ray_tree_build, untouched (any order of the records).
 *
 * THE PAIR.  Record (a, e1, e2), point q, x . y = fma(x_z, y_z, fma(x_y, y_y, x_x y_x)); fp32 throughout, IEEE divisions, no
 *   contraction: every fused operation is one of the fma written here, va, vb, vc are two products and one subtraction.
 *   The region walk of Ericson, Real-Time Collision Detection 5.1.5; the FIRST region that applies wins:
 *     ap = q - a;  d1 = e1 . ap, d2 = e2 . ap                     d1 <= 0 and d2 <= 0                 -> (u, v) = (0, 0)
 *     bp = ap - e1; d3 = e1 . bp, d4 = e2 . bp                    d3 >= 0 and d4 <= d3                -> (1, 0)
 *     vc = d1 d4 - d3 d2                                          vc <= 0, d1 >= 0, d3 <= 0           -> (d1 / (d1 - d3), 0)
 *     cp = ap - e2; d5 = e1 . cp, d6 = e2 . cp                    d6 >= 0 and d5 <= d6                -> (0, 1)
 *     vb = d5 d2 - d1 d6                                          vb <= 0, d2 >= 0, d6 <= 0           -> (0, d2 / (d2 - d6))
 *     va = d3 d6 - d5 d4;  w = (d4 - d3) / ((d4 - d3) + (d5 - d6))
 *                                                                 va <= 0, d4 - d3 >= 0, d5 - d6 >= 0 -> (1 - w, w)
 *     otherwise  den = 1 / ((va + vb) + vc), u = vb den, v = vc den, then clamped by comparisons that leave a NaN alone:
 *                u < 0 -> 0, u > 1 -> 1, v < 0 -> 0, v > 1 - u -> 1 - u
 *     r_x = fma(-v, e2_x, fma(-u, e1_x, ap_x)) (y, z alike);  dist2 = r . r;  the closest point is a + u e1 + v e2.
 *   The clamp of the last region is this build's addition to Ericson: in exact arithmetic it does nothing; in fp32 it keeps
 *   (u, v) inside u >= 0, v >= 0, u + v <= 1 + 2^-24 whatever cancellation did to va, vb, vc on a sliver, so the point lies
 *   on the triangle in EVERY region, which the culling bound below needs.  A record with e1 = e2 = 0 (all six +-0) takes no
 *   part: a triangle collapsed to a point, which is how the tree stores an invalid row and the padding (a wave-uniform
 *   test: records come through scalar loads).  A NaN dist2 never wins, every comparison with it being false: a collinear
 *   triangle that reaches the last line with 0 x inf, a non-finite coordinate of the record (it is multiplied into r in
 *   every region, 0 x inf included) or of q.  A dist2 that overflowed to +inf does not win either.
 * RESULT.  Per point the smallest (dist2 bits, face_of) in full key order over ALL records that take part: dist2_out [nq],
 *   face_out [nq] the ORIGINAL face index, bary_out [nq,2] = (u, v) of the winner (may be NULL).  No winner: (+inf, -1, (0, 0)).
 * THE INVARIANT.  flags = 0 returns, for every point, bit for bit what FGC_CP_EXHAUSTIVE returns (no culling: every point
 *   tests every record, nq x nf pairs - the brute force, through the same kernel with every bound taken as 0).  Hence the
 *   result of a point is a function of the mesh and that point alone: not of the order of the records or of the points, the
 *   neighbours in the wave, the launch geometry, eager or replayed.
 * THE BOUND of a lane's point against a box (lo, hi): per axis g = max(lo - q, q - hi, 0) taken by comparisons that keep a
 *   NaN, g' = max(g - 2^-18 max(|lo|, |hi|, |q|), 0); s = g'_x^2 + g'_y^2 + g'_z^2 summed in that order;
 *   lb = max(s - (s 2^-21 + 2^-125), 0).  The lane takes part in the box iff lb <= best dist2 and lb < inf, non-strict: an
 *   equal dist2 on a lower face index inside a box at exactly best is still found.  A box is skipped only if lb > best.
 *   Why lb never exceeds the COMPUTED dist2 of a record in the box.  The box holds the original vertices a, b, c exactly
 *   (min / max), so on every axis |a|, |b|, |c| <= B = max(|lo|, |hi|) and, with M = max(B, |q|): |e1|, |e2| <= 2B(1 + 2^-24),
 *   each within 2^-24 2B of b - a, c - a.  (u, v) lies in the triangle of the parameter plane up to 2^-24 (every region,
 *   thanks to the clamp), so p = a + u e1 + v e2 taken exactly lies within 2^-24 4B(1 + ..) of the real triangle, which is
 *   inside the box: |q - p| >= g - 2^-22 B(1 + ..), g taken exactly; the computed g adds 2^-24 2M.  The computed r is
 *   q - p up to three roundings (the subtraction, two fma) of intermediates no larger than |q| + |a| + |e1| + |e2| <= 6M(1 + ..):
 *   18 x 2^-24 M.  Together below 25 x 2^-24 M per axis - absolute, in units of the coordinates, NOT relative to the distance:
 *   a point near the surface has g ~ 0 and the full error.  The slack 2^-18 M is 64 x 2^-24 M.  So g' <= |computed r| on
 *   every axis; the three squares and two sums of s round up by at most (1 + 2^-24)^3, r . r rounds down by at most as
 *   much, and 2^-21 (and 2^-125 for a sum that underflowed) is more than both: lb <= dist2.  Over-visiting a few boxes
 *   costs nothing measurable; losing the winner is a wrong answer.  An empty box (+inf, -inf) gives inf - inf, a NaN, which
 *   no comparison admits; so does a point with a NaN.  Records the tree keeps out of every box (a non-finite vertex) have a
 *   NaN dist2 and win nothing under FGC_CP_EXHAUSTIVE either.
 * THE WALK is fgc_ray_cast_tree's: one wave of 64 points per workgroup, a wave-uniform stack of (node, ballot) entries in
 *   LDS, boxes and records through scalar loads; a lane takes part in a node only while its own bound allows, with the best
 *   it has at that moment.  The children of a node are visited NEAREST-FIRST by the wave's smallest lb over the lanes that
 *   take part, among equal lb (a point near the surface lies inside several boxes: lb = 0) by the smallest squared distance
 *   to the middle of the box, then by index; the farthest is pushed first.  Before the search the wave walks the tree once
 *   greedily - every lane follows only its own nearest child by that order, down to one leaf - so that each lane starts
 *   the search with a finite best of its own neighbourhood.  By the invariant, the order and the first walk change the
 *   time and not one bit (the first walk only tests pairs the search may test again).  A lane beyond nq holds the last
 *   point and stores nothing.  NO LOOP ENDS ON DEVICE DATA: a walk pushes each node at most once, so each of the two pops at most (number of
 *   nodes) times, a host-side count; the stack holds at most 7 entries per level + 1; every popped id is bounded before
 *   it addresses anything.  One launch, no atomics, no workspace, enqueue-only, capturable.
 * A NULL among tree, points, dist2_out, face_out; nf or nq <= 0; nf > FGC_RAY_CAST_MAX_FACES; flag bits other than
 *   FGC_CP_EXHAUSTIVE; a tree that is misaligned or below fgc_ray_tree_bytes(nf): FGC_EINVAL, nothing launched. */
#define FGC_CP_EXHAUSTIVE 1u
int fgc_closest_point_tree(const void* tree, size_t tree_bytes, int32_t nf, const float* points, int32_t nq, uint32_t flags,
                           float* dist2_out, int32_t* face_out, float* bary_out, void* stream);

/* The same query without a tree, over all nq x nf pairs: what fgc_ray_cast is to fgc_ray_cast_tree.  For a mesh that moves
 * every step (fgc_surface_loss), where a build per step costs more than a thousand points save.
 *   verts [nv,3], faces [nf,3], points [nq,3]; dist2_out [nq], face_out [nq], bary_out [nq,2] (may be NULL) as above.
 *   Records are fgc_ray_cast's: a row with a vertex id outside [0, nv) is a zero record and takes no part, which covers the
 *   -1 rows of a node-ordered face table.  THE PAIR is the one function above; the winner is the smallest
 *   (dist2 bits, face) in full key order; a NaN and +inf never win; no winner: (+inf, -1, (0, 0)).
 * THE CONTRACT.  Every output is bit for bit what fgc_closest_point_tree returns on a tree of the same mesh (any order):
 *   the same records, the same per-pair function, an exact minimum - each workgroup's result goes into a 64-bit integer
 *   atomic min on (float bits of dist2) << 32 | face, and dist2 >= 0 orders like its bits - so the result does not depend on
 *   how the launch splits points and faces, and is the same bits eager or replayed.  No floating-point atomics.
 * workspace (device, 16-byte aligned) >= fgc_closest_point_workspace_bytes(nf, nq) (0 for arguments out of range):
 *   fgc_ray_cast's layout, the records and one 64-bit key per point.
 * Three launches, enqueue-only, capturable, nothing allocated: the records (and the keys' initial value); points x faces
 *   (64 points per workgroup, the records wave-uniform through scalar loads, the faces split into slabs over blockIdx.y
 *   where the points alone do not fill the device, one atomic per point and slab); keys -> outputs, (u, v) evaluated again
 *   on the winner, whose index is bounded by nf before it addresses anything.  Every loop bound is a host-side count.
 * A NULL among verts, faces, points, dist2_out, face_out, workspace; nv, nf or nq <= 0; nf > FGC_RAY_CAST_MAX_FACES; a
 *   workspace that is misaligned or too small: FGC_EINVAL, nothing launched. */
size_t fgc_closest_point_workspace_bytes(int32_t nf, int32_t nq);
int fgc_closest_point(const float* verts, int32_t nv, const int32_t* faces, int32_t nf, const float* points, int32_t nq,
                      float* dist2_out, int32_t* face_out, float* bary_out, void* workspace, size_t workspace_bytes,
                      void* stream);

/* Two-sided point-to-surface loss, shaped like fgc_point_loss, and its gradient: the ground truth may be a mesh of any
 * topology.  p0 [np0,3] refined vertices with faces0 [nf0,3] (-1 rows allowed: a node-ordered table), p1 [np1,3] and
 * faces1 [nf1,3] the ground-truth mesh, i0 [ns0] rows of p0 and i1 [ns1] rows of p1 (repeats allowed):
 *   precision_t = distance of p0[i0_t] to the surface (p1, faces1), completeness_t = distance of p1[i1_t] to the surface
 *   (p0, faces0), each d = sqrtf(dist2) of the winner of fgc_closest_point;
 *   loss[0] = 1000 (mean(d <= threshold ? d : 0 over precision) + mean(the same over completeness)): fgc_point_loss's scale.
 * g_p0 (may be NULL) [np0,3] receives dL/dp0 (dL/dloss = 1), with r = q - closest point as THE PAIR forms it and (u, v) of
 *   the winner held fixed: a kept precision term adds (1000/ns0) r / d to row i0_t; a kept completeness term adds
 *   -(1000/ns1) w_k r / d to the three rows faces0[f][k] of its winning face, w = (1 - u - v, u, v).  Holding (u, v) fixed is
 *   exact wherever the distance is differentiable: the closest point minimises over the triangle, so the derivative
 *   through (u, v) vanishes.  At d = 0 a term's gradient is 0; a masked term's gradient is 0.  Terms that share a row are
 *   summed in term order by the row's first term - precision terms first, then completeness terms in the order (t, k) - by
 *   fgc_point_loss's reduction: no atomics on floats, the same bits from run to run and under hipGraph replay.
 * A sample index out of range, or a sample with no winner, makes the loss NaN and adds no gradient.
 * ns0 + 3 ns1 <= FGC_POINT_LOSS_MAX_SAMPLES.  workspace (device, 256-byte aligned) >=
 *   fgc_surface_loss_workspace_bytes(nf0, nf1, ns0, ns1) (0 for arguments out of range).  Enqueue-only, capturable: two
 *   gathers, two scans of two launches, the terms, a memset of g_p0, the reduction.  A NULL among the pointers other than
 *   g_p0; a count <= 0; too many samples or faces; a workspace that is misaligned or too small: FGC_EINVAL, nothing
 *   launched. */
size_t fgc_surface_loss_workspace_bytes(int32_t nf0, int32_t nf1, int32_t ns0, int32_t ns1);
int fgc_surface_loss(const float* p0, int32_t np0, const int32_t* faces0, int32_t nf0, const float* p1, int32_t np1,
                     const int32_t* faces1, int32_t nf1, const int32_t* i0, int32_t ns0, const int32_t* i1, int32_t ns1,
                     float threshold, float* loss, float* g_p0, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Checkpoint files (CPU; HOST pointers)
 * ---------------------------------------------------------------------------------- */

/* CRC-32C (Castagnoli, reflected polynomial 0x82F63B78) of data[0..n) continued from crc (0 to start): the
 * checksum of the TensorFlow tensor-bundle files tf.train.Saver writes and restores (train.py:79-87,522-534,
 * 551-552): every block of `<prefix>.index` and every tensor of `<prefix>.data-*` carries it.  Unmasked value. */
uint32_t fgc_crc32c(uint32_t crc, const void* data, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* FGC_H */
