/*
 * dw_hip.h — C ABI of the MI355X (gfx950) DeepWalk / node2vec hot path.
 *
 * The reference (Robotmurlock/Deepwalk-and-Node2vec) is pure Python and has no FFI; each entry
 * point below replaces one Python call surface of its two hot paths:
 *
 *   path A (walks):  shallow_encoders/graph/random_walk_generator.py:41-119
 *   path B (SGNS):   shallow_encoders/word2vec/model.py:79-91, loss.py:14-22,
 *                    utils/sampling.py:7-21, trainer.py:131-152, + torch.optim.Adam step
 *
 * Conventions (every function):
 *   - all array arguments are DEVICE pointers owned by the caller (torch tensors' data_ptr());
 *     no function allocates user-visible memory;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     every launch is stream-ordered and asynchronous;
 *   - functions are stateless and reentrant (distinct buffers ⇒ safe from several host threads);
 *   - return value: DW_OK (0) or a negative DW_E_* code; dw_last_error_string() (thread-local)
 *     describes the last failure. Nothing throws or aborts across the ABI;
 *   - conditions found ON THE DEVICE (an isolated node met by a walker, a rejection loop that
 *     exceeded its bound, a bad CSR entry) are OR-ed into the caller's int32 `status` word
 *     (DW_S_* bits) so the host can check them when it next synchronises.
 *
 * Graph layout in HBM (CSR, vocabulary ids: row 0 is `<unk>` with no neighbours, node i of the
 * vocabulary is row i; neighbour order = networkx `graph.neighbors()` insertion order):
 *   row_ptr int64[n_rows+1], col int32[nnz], weights float64[nnz] (NULL = unweighted),
 *   col_sorted int32[nnz] (each row's neighbours sorted ascending, for adjacency tests).
 */
#ifndef DW_HIP_H
#define DW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- return codes ---------------------------------------------------------------------- */
#define DW_OK                0
#define DW_E_INVALID_ARG    -1
#define DW_E_HIP            -2
#define DW_E_UNSUPPORTED    -3

/* ---- device status bits (OR-ed into the caller's int32 status word) -------------------- */
#define DW_S_ISOLATED_NODE   1   /* walker reached a node with no neighbours (reference: IndexError) */
#define DW_S_ZERO_WEIGHT     2   /* all neighbour weights zero (reference: ZeroDivisionError)        */
#define DW_S_REJECTION_CAP   4   /* node2vec rejection exceeded DW_MAX_REJECTION_ROUNDS              */
#define DW_S_BAD_CSR         8   /* row_ptr not monotone / col out of range                          */
#define DW_S_BAD_INDEX      16   /* an index outside [0, V) reached the SGNS kernel                  */
#define DW_S_RECORDS_FULL   32   /* owner-form SGNS records exceeded the workspace (not expected)    */
#define DW_S_DUP_NEIGHBOR   64   /* a CSR row lists a neighbour twice (dw_csr_check_simple)          */
#define DW_S_FIXED_RANGE   128   /* a gradient term past the deterministic fixed-point range         */
#define DW_S_BAD_TEXT      256   /* a line of an edge-list text is malformed (dw_edgelist_parse*)    */
#define DW_S_NEG_WEIGHT    512   /* a negative edge weight reached dw_alias_build (no table law)     */
#define DW_S_NAN_SCORE    1024   /* a NaN score reached dw_roc_auc (it has no rank)                  */
#define DW_S_NONFINITE    2048   /* a nan or inf value reached the embedding text writer             */
#define DW_S_FOREST_ROUNDS 4096  /* dw_edge_forest's last allowed round still joined components      */
#define DW_S_TEXT_KEY     8192   /* the embedding text reader met a key that is no plain integer    */

#define DW_METHOD_DEEPWALK   0   /* random_walk_generator.py:56-72 ('deepwalk' and 'dfs')          */
#define DW_METHOD_NODE2VEC   1   /* random_walk_generator.py:75-119                                  */

#define DW_MAX_REJECTION_ROUNDS 65536
#define DW_ADJ_HASH_MIN_DEG  8   /* rows of higher degree get an adjacency hash (dw_adj_hash_*)        */

/* ---- library ---------------------------------------------------------------------------- */
const char *dw_last_error_string(void);
int dw_abi_version(void);               /* bumps on any signature change */
/* SHA-256 prefix (16 hex digits) of the sources the library was built from (csrc/build.py
 * source_id): a shipped binary can be checked against the tree it came with. */
const char *dw_build_id(void);
int dw_device_sync(void *stream);       /* hipStreamSynchronize(stream); used by the host mirror */
/* dst = src, bytes a multiple of 16 (16-B aligned device buffers): a STREAM-copy kernel, the
 * measured HBM roofline bench.py reports beside the spec peak. */
int dw_stream_copy(const void *src, void *dst, int64_t bytes, void *stream);

/* Host-side (no device work): CPython 3.10 random.shuffle over range(n), bit for bit — the
 * reference's start-node shuffle (datasets.py:45,86-88) in native code. mt_state: the 625 words
 * of random.getstate()[1] (624-word MT19937 state + index), advanced in place exactly as
 * Python's shuffle would; perm: int64[n] out. */
int dw_host_shuffle(uint32_t *mt_state, int64_t *perm, int64_t n);

/* ---- the reference's uniform stream on the device ------------------------------------------
 * CPython's random.random() (Modules/_randommodule.c: MT19937 + genrand_res53), the one draw per
 * walk step of random_walk_generator.py:68,113 (random.choices(..., k=1)); replaces the host
 * draw + H2D copy in front of dw_walk_replay(_inline). Replaces, in the reference,
 * `random.random()` called n times on the global generator (datasets.py:87-91 -> walk()).
 *
 * dw_mt_jump_table (HOST, no device work): jump-ahead polynomials for dw_mt_uniforms. Chain c
 * (c >= 1) of a call starts at raw word 624*window_stride*c of the generator's sequence; its
 * entry lists the exponents l (ascending) of t^(624*window_stride*c - 2) mod phi(t), phi =
 * MT19937's characteristic polynomial (degree 19937, 135 terms). offsets: int64[n_chains+1]
 * (chain c's exponents are positions[offsets[c] .. offsets[c+1])); positions: uint16[capacity]
 * (n_chains * 19937 always suffices; DW_E_INVALID_ARG when too small). Host buffers.
 *
 * dw_mt_uniforms: out[k] = the (k+1)-th random.random() of the generator whose state is
 * (mt[0..623], index) — random.getstate()[1] — for k < n; state_out (625 words: array + index)
 * receives the state after the n draws, for random.setstate. mt, out, state_out, jump_pos,
 * jump_off, workspace: DEVICE buffers (jump_*: a dw_mt_jump_table of the same window_stride
 * with at least chains = ceil(windows / window_stride) entries, windows = (index + 2n - 1) / 624
 * + 1; workspace: dw_mt_workspace_words(chains) uint32 words; all may be NULL when that is one
 * chain). Two stream-ordered launches: the chains' jumps, then one workgroup per chain. */
int dw_mt_jump_table(int64_t window_stride, int64_t n_chains, int64_t *offsets,
                     uint16_t *positions, int64_t capacity);
int dw_mt_uniforms(const uint32_t *mt, int32_t index, int64_t n, double *out,
                   uint32_t *state_out, int64_t window_stride, const uint16_t *jump_pos,
                   const int64_t *jump_off, int64_t n_chains_table, uint32_t *workspace,
                   int64_t workspace_words, void *stream);
int64_t dw_mt_workspace_words(int64_t n_chains);

/* A generator whose state lives in HBM (state: 625 uint32 words, the 624-word array + the
 * index, random.getstate()[1]'s layout; torch's CPU generator maps onto the same layout), advanced
 * in place by n draws (through scratch, 625 words, then copied back; stream-ordered and
 * capturable in a HIP graph):
 *   mode 0: out float64[n] = the next n random.random() (as dw_mt_uniforms);
 *   mode 1: out int64[n] = the next n torch.randint(0, range, ...) values of torch's CPU
 *           generator for range < 2^28 (aten's mt19937, one 32-bit output per value,
 *           `% range`) — generate_noise_batch (utils/sampling.py:7-21), noise='torch';
 *   mode 2: the same for 2^28 <= range < 2^32, where torch takes two outputs per value
 *           ((first << 32 | second) % range).
 * index >= 0: the host knows the index (it must equal state[624]), the launch is sized to it;
 * index < 0: read on the device (a replayed graph), the launch covers the largest index.
 * jump_* / workspace as dw_mt_uniforms for chains = ceil(windows / window_stride), windows =
 * (index + w n - 1) / 624 + 1, w = 1 (mode 1) or 2, index = 624 when read on device. */
int dw_mt_draw(int32_t mode, uint32_t *state, int32_t index, int64_t n, void *out,
               uint64_t range, uint32_t *scratch, int64_t window_stride,
               const uint16_t *jump_pos, const int64_t *jump_off, int64_t n_chains_table,
               uint32_t *workspace, int64_t workspace_words, void *stream);

/* ---- graph ------------------------------------------------------------------------------- */

/* Validate a CSR on the device: row_ptr[0]==0, monotone, row_ptr[n_rows]==nnz, 0<=col<n_rows.
 * Replaces nothing in the reference (networkx guarantees it); guards every kernel below. */
int dw_csr_validate(const int64_t *row_ptr, const int32_t *col, int64_t n_rows, int64_t nnz,
                    int32_t *status, void *stream);

/* Sorted copy of every neighbour list (ascending ids), used for the node2vec adjacency test
 * `prev_node in candidate_neighbors` (random_walk_generator.py:106-107).
 * Two-phase temp-storage protocol: call with temp==NULL to get *temp_bytes, then again. */
int dw_csr_sort_copy(const int64_t *row_ptr, const int32_t *col, int64_t n_rows, int64_t nnz,
                     int32_t *col_sorted, void *temp, size_t *temp_bytes, void *stream);

/* Sets DW_S_DUP_NEIGHBOR in status when a row of col_sorted (dw_csr_sort_copy) holds two equal
 * entries. The reference's networkx.Graph keeps one entry per neighbour
 * (random_walk_generator.py:41-42 lists graph.neighbors(node)), and the bit-exact node2vec replay
 * relies on it (one position of prev in N(v), class counts by intersection), so the host refuses a
 * non-simple CSR there. */
int dw_csr_check_simple(const int64_t *row_ptr, const int32_t *col_sorted, int64_t n_rows,
                        int64_t nnz, int32_t *status, void *stream);

/* Per-row adjacency hash for the fast node2vec walker's test `prev_node in
 * candidate_neighbors` (random_walk_generator.py:106-107): one probe of a 64-B bucket instead of
 * a ceil(log8 deg)-load search of the sorted list. A row u of degree > DW_ADJ_HASH_MIN_DEG owns
 * nb = ceil(4 deg / 48) buckets of 16 int32 slots (load <= 3/4) at adj_hash + adj_off[u]; rows
 * of lower degree own none (their neighbour list itself is one load).
 *   dw_adj_hash_offsets: adj_off int64[n_rows + 1] (exclusive scan of the per-row slot counts;
 *     adj_off[n_rows] = total slots). Two-phase temp protocol as dw_csr_sort_copy.
 *   dw_adj_hash_build: fills adj_hash int32[n_slots] (n_slots = adj_off[n_rows]). */
int dw_adj_hash_offsets(const int64_t *row_ptr, int64_t n_rows, int64_t *adj_off, void *temp,
                        size_t *temp_bytes, void *stream);
int dw_adj_hash_build(const int64_t *row_ptr, const int32_t *col, int64_t n_rows,
                      const int64_t *adj_off, int64_t n_slots, int32_t *adj_hash, int32_t *status,
                      void *stream);
/* adj_hpos int32[n_slots]: for every filled slot of adj_hash, the index of its key in the row's
 * neighbour order (-1 for free slots) — the bit-exact node2vec replay's position lookups
 * (dw_walk_replay_indexed). After dw_adj_hash_build. */
int dw_adj_hash_positions(const int64_t *row_ptr, const int32_t *col, int64_t n_rows,
                          const int64_t *adj_off, const int32_t *adj_hash, int64_t n_slots,
                          int32_t *adj_hpos, int32_t *status, void *stream);

/* Per-row Vose alias tables for first-order weighted sampling (the fast-mode replacement of
 * get_node_normalized_edge_weights + random.choices, random_walk_generator.py:50-53,68).
 * prob_thr[e] = floor(P_accept * 2^32) clamped to [0, 2^32-1] with 2^32-1 meaning "always";
 * alias[e] = local index (0..deg-1) of the alias entry. A row whose weights do not sum to a
 * positive number sets DW_S_ZERO_WEIGHT, a row holding a negative weight DW_S_NEG_WEIGHT; such a
 * row gets the identity table and the caller must not walk with the result.
 * work_prob float64[nnz], work_idx int32[nnz]: caller-provided scratch. */
int dw_alias_build(const int64_t *row_ptr, const double *weights, int64_t n_rows, int64_t nnz,
                   uint32_t *prob_thr, int32_t *alias, double *work_prob, int32_t *work_idx,
                   int32_t *status, void *stream);

/* ---- walks -------------------------------------------------------------------------------- */

/* ---- Graph ingestion on the device (shallow_encoders/graph/rmat.py) ----
 * R-MAT edge draws replacing rmat.py:rmat_edges' numpy loop: the uniforms are numpy's
 * default_rng PCG64 stream, draw index level * n_edges + edge. The host supplies level_state
 * (2*scale uint64: lo, hi of the 128-bit state before level l's first draw), jump (64 x 4
 * uint64: multiplier lo/hi, increment lo/hi of 2^i steps), the stream increment and the
 * thresholds t1 = a, t2 = a + b, t3 = a + b + c. Output: edges packed (src << 32 | dst),
 * self-loops dropped, undirected duplicates removed keeping the first draw, in draw order;
 * *n_unique (device int64) = their count. Workspace >= dw_ingest_workspace_bytes. */
int dw_ingest_workspace_bytes(int32_t scale, int64_t n_edges, int64_t n_nodes, size_t *bytes);
int dw_rmat_edges(int32_t scale, int64_t n_edges, const uint64_t *level_state,
                  const uint64_t *jump, uint64_t inc_lo, uint64_t inc_hi, double t1, double t2,
                  double t3, uint64_t *edges, int64_t *n_unique, void *workspace,
                  size_t workspace_bytes, void *stream);

/* Nodes of [0, n_nodes) that no edge touches, increasing (rmat.py's isolated-node patch list);
 * *n_isolated is a device int64. Endpoints >= n_nodes set DW_S_BAD_CSR. */
int dw_graph_isolated(const uint64_t *edges, int64_t n_edges, int64_t n_nodes,
                      int32_t *isolated, int64_t *n_isolated, int32_t *status, void *workspace,
                      size_t workspace_bytes, void *stream);

/* CSR of an undirected packed edge list (rmat.py:csr_from_edges / networkx add_edges_from
 * order): row_ptr int64 [n_nodes + 2] (row 0 = <unk>, row i+1 = node i), col int32
 * [2 n_edges] holding vocabulary ids (node + 1); each row lists its edges in edge order. */
int dw_csr_from_edges(const uint64_t *edges, int64_t n_edges, int64_t n_nodes,
                      int64_t *row_ptr, int32_t *col, int32_t *status, void *workspace,
                      size_t workspace_bytes, void *stream);

/* ---- Edge-list ingestion (shallow_encoders/graph/edge_list.py): a user's graph, as text or as
 * id arrays, to the CSR of CSRGraph.from_networkx(nx.Graph().add_edges_from(...)) over names
 * "n" + zero-padded id. One workspace size serves the three calls below (n_text_bytes: the
 * largest text chunk, 0 without text; n_edges: the largest raw edge count). Every output is a
 * pure function of the input (stable sorts, scans, selects, integer atomics only). */
int dw_edgelist_workspace_bytes(int64_t n_text_bytes, int64_t n_edges, size_t *bytes);

/* Parses text[0, n_bytes) (uint8, in HBM; no read goes past n_bytes), one edge per line: lines end
 * in '\n' (a '\r' that closes the line is dropped, the last line may lack its '\n'); lines of
 * blanks (space, tab) only, and lines whose first non-blank byte is '#' or '%', are skipped; a
 * data line is blanks, 1-18 decimal digits, one or more of {space, tab, comma}, 1-18 digits,
 * then the line's end or a separator followed by anything. Lines with index < skip_lines are
 * dropped unparsed. Output: src, dst int64 [capacity] in file order (a data line past capacity
 * sets DW_S_RECORDS_FULL; capacity (n_bytes + 1) / 4 always suffices), counts[0] = data lines,
 * counts[1] = lines seen (device int64 [2]). Any other line sets DW_S_BAD_TEXT and
 * *err_line (device int64) = the smallest such 0-based line index, else -1. */
int dw_edgelist_parse(const uint8_t *text, int64_t n_bytes, int64_t skip_lines, int64_t *src,
                      int64_t *dst, int64_t capacity, int64_t *counts, int64_t *err_line,
                      int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* dw_edgelist_parse for "u v w" lines: behind the second id a data line needs one or more
 * separators and a weight token, then the line's end or a separator followed by anything. The
 * token: [+-], then digits [. digits*] or . digits+, then optionally e|E [+-] 1-4 digits; at most
 * 64 bytes; no nan, inf, hex or '_'. Every other line (no third field included) is DW_S_BAD_TEXT.
 * weight float64 [capacity] gets float(token) bit for bit, converted in integer arithmetic
 * (Eisel-Lemire over pow5: device uint64 [1302], the words of dw_pow5_table), except for
 * undecided tokens — more than 19 significant digits whose rounding the first 19 do not fix, a
 * product whose low bits do not, a subnormal, underflowing or overflowing value: those get 0.0
 * and an entry (edge index, byte offset of the token) in undecided (device int64
 * [2 undecided_capacity], in no particular order; entries past the capacity are dropped but
 * counted) for the host to convert. counts (device int64 [3]): data lines, lines seen, undecided
 * tokens. The workspace is dw_edgelist_parse's (dw_edgelist_workspace_bytes). */
int dw_edgelist_parse_weighted(const uint8_t *text, int64_t n_bytes, int64_t skip_lines,
                               const uint64_t *pow5, int64_t *src, int64_t *dst, double *weight,
                               int64_t capacity, int64_t *undecided, int64_t undecided_capacity,
                               int64_t *counts, int64_t *err_line, int32_t *status,
                               void *workspace, size_t workspace_bytes, void *stream);

/* Host only (no device needed). The table dw_edgelist_parse_weighted reads: for q = -342 .. 308
 * the (high, low) 64-bit words of a 128-bit approximation of 5^q with bit 127 set — q >= 0: the
 * top 128 bits of 5^q, truncated; q < 0: floor(2^(b + 127) / 5^-q) + 1, b = bit length of 5^-q.
 * Computed once with exact integer arithmetic. out: host uint64 [1302]. */
int dw_pow5_table(uint64_t *out);

/* Host only: the kernel's token scan and conversion on token[0, n_bytes) (a testing aid).
 * *kind = DW_TOKEN_BAD (not a weight token), DW_TOKEN_DECIDED (*bits = the double's bits) or
 * DW_TOKEN_UNDECIDED. */
#define DW_TOKEN_BAD       0
#define DW_TOKEN_DECIDED   1
#define DW_TOKEN_UNDECIDED 2
int dw_weight_token_host(const uint8_t *token, int64_t n_bytes, int32_t *kind, uint64_t *bits);

/* ---- Embeddings to word2vec text (shallow_encoders/word2vec/embeddings_io.py): line r is
 * "<key r> <T(v_0)> .. <T(v_{dim-1})>\n" for row rows[r] of table (float32 [vocab_size, dim];
 * rows int64 [n_rows], NULL = rows 0 .. n_rows - 1), single spaces, no '\r'. The key is
 * keys_i64[r] in plain decimal (int64 [n_rows], >= 0) or the bytes key_bytes[key_off[r],
 * key_off[r + 1]) (key_off int64 [n_rows + 1]); exactly one of the two forms is given. T(x) is the
 * shortest decimal that rounds back to the float32 x, laid out as CPython's repr(float) lays out
 * a double with those digits ("0.0", "-0.0", "0.0001", "1e-05", "9999999000000000.0", "1e+16";
 * "nan", "inf", "-inf"); at most 19 bytes. It is computed in integer arithmetic alone (Ryu for
 * binary32 over tab: uint64 [79], the words of dw_f32text_table). A row id outside
 * [0, vocab_size) sets DW_S_BAD_INDEX and prints as zeros, a negative key sets it and prints as
 * 0; a nan or inf value sets DW_S_NONFINITE (its token is still written). dim > 512 returns
 * DW_E_UNSUPPORTED before any launch. Every output is a pure function of the input. */

/* Host only: the 79 words the conversion reads — for q = 0 .. 30 floor(2^(b(q) - 1 + 59) / 5^q)
 * + 1, then for i = 0 .. 47 the top 61 bits of 5^i (b = the bit length of the power), computed
 * with exact integers. out: host uint64 [79]. */
int dw_f32text_table(uint64_t *out);

/* Host only (no device; every pointer is host memory): both passes below in one entry point, the
 * CPU path of save_word2vec_format and the kernels' mirror for tests. out == NULL: writes line_off
 * [n_rows + 1] and ORs the status bits of all rows into *status (r0, r1, capacity ignored).
 * out != NULL: writes the lines of rows [r0, r1) at out + line_off[r] - line_off[r0];
 * DW_E_INVALID_ARG, with nothing written, when they need more than capacity bytes. */
int dw_embtext_host(const float *table, int64_t vocab_size, int32_t dim, const int64_t *rows,
                    int64_t n_rows, const int64_t *keys_i64, const uint8_t *key_bytes,
                    const int64_t *key_off, int64_t *line_off, int64_t r0, int64_t r1,
                    uint8_t *out, int64_t capacity, int32_t *status);

int dw_embtext_workspace_bytes(int64_t n_rows, int32_t dim, size_t *bytes);

/* Pass 1: line_off (device int64 [n_rows + 1]) = the exclusive scan of the lines' byte lengths,
 * the total in its last entry; the status bits above. */
int dw_embtext_sizes(const float *table, int64_t vocab_size, int32_t dim, const int64_t *rows,
                     int64_t n_rows, const int64_t *keys_i64, const uint8_t *key_bytes,
                     const int64_t *key_off, const uint64_t *tab, int64_t *line_off,
                     int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* Pass 2: the lines of rows [r0, r1) into out (device uint8 [capacity]) at line_off[r] -
 * line_off[r0], with the inputs and the line_off of pass 1. When line_off[r1] - line_off[r0]
 * exceeds capacity nothing is written and DW_S_RECORDS_FULL is set (line_off lives on the
 * device: the launch does not wait for it). No byte at or past line_off[r1] - line_off[r0] is
 * stored, and no line stores outside its own [line_off[r], line_off[r + 1]). */
int dw_embtext_write(const float *table, int64_t vocab_size, int32_t dim, const int64_t *rows,
                     int64_t n_rows, const int64_t *keys_i64, const uint8_t *key_bytes,
                     const int64_t *key_off, const uint64_t *tab, const int64_t *line_off,
                     int64_t r0, int64_t r1, uint8_t *out, int64_t capacity, int32_t *status,
                     void *stream);

/* ---- Word2vec text to embeddings (embeddings_io.read_word2vec_format), the way back: text[0,
 * n_bytes) (uint8, at any alignment; no read goes past n_bytes or in front of text) is the body
 * of a word2vec text file, or a run of whole lines of it — the caller reads the "<n> <d>" header.
 * Lines end in '\n'; the last line may lack it. A line's tokens are its maximal runs of bytes
 * other than space, \t, \v, \f and \r (what bytes.split() splits on: a '\r' that closes a line is
 * dropped). Line l of the text is row row0 + l of the outputs; it holds a key and dim value
 * tokens:
 *   - key_off, key_len (int64 [n_rows]): the key's byte span in text; key_i64 (int64 [n_rows]):
 *     its value where the key is 1 to 18 decimal digits with no sign and no leading zero but "0"
 *     itself (str(value) gives the bytes back), else -1, and DW_S_TEXT_KEY is set;
 *   - value token j goes to table[row, j] (float32 [n_rows, dim]) as numpy.float32(float(token)):
 *     the double nearest the decimal (dw_edgelist_parse_weighted's grammar and conversion over
 *     pow5), then that double rounded to float32, ties to even, in integer arithmetic — subnormal
 *     results, the round-up into FLT_MIN, +-inf from 2^128 - 2^103 on, +-0. nan, inf and infinity,
 *     in any letter case and with an optional sign, give 0x7FC00000 / 0x7F800000 with the sign
 *     bit. Every other token — one the conversion cannot decide, one of more than 64 bytes, one
 *     outside the grammar ("1_0", "0x10", "1e12345", "abc") — is undecided: 0.0 in the table and
 *     an entry (row, column, byte offset, byte length) in undecided (int64 [4
 *     undecided_capacity], in no particular order; entries past the capacity are dropped but
 *     counted) for the host's float() to convert or refuse.
 * A line whose token count is not dim + 1 (an empty or all-blank one included) sets
 * DW_S_BAD_TEXT and lowers *err_line (int64, -1 = none) to the smallest such 0-based line of the
 * text; nothing of it is stored. counts (int64 [2]): lines of the text, undecided tokens. dim >
 * 512 returns DW_E_UNSUPPORTED before any launch. Every output is a pure function of the input
 * (integer atomics only: the undecided counter, the error line, the status word). */

/* Host only (no device; every pointer is host memory): both passes below in one entry point, the
 * CPU path of read_word2vec_format and the kernels' mirror for tests. Lines behind row n_rows - 1
 * are counted, not parsed. */
int dw_embread_host(const uint8_t *text, int64_t n_bytes, int32_t dim, float *table,
                    int64_t n_rows, int64_t row0, int64_t *key_off, int64_t *key_len,
                    int64_t *key_i64, int64_t *undecided, int64_t undecided_capacity,
                    int64_t *counts, int64_t *err_line, int32_t *status);

/* Host only: the reader's value-token conversion on token[0, n_bytes) (a testing aid). *kind =
 * DW_TOKEN_BAD (empty, or it holds a blank), DW_TOKEN_DECIDED (*bits32 = the float32's bits) or
 * DW_TOKEN_UNDECIDED. */
int dw_f32_token_host(const uint8_t *token, int64_t n_bytes, int32_t *kind, uint32_t *bits32);

int dw_embread_workspace_bytes(int64_t n_bytes, size_t *bytes);

/* Pass 1, the line index: line_off (device int64 [capacity + 1]) = the byte offsets of the line
 * starts, and the text's end behind the last line; entries of lines past capacity are not
 * written. Sets counts[0] = lines (compare it with the header's n before pass 2), counts[1] = 0
 * and *err_line = -1. */
int dw_embread_lines(const uint8_t *text, int64_t n_bytes, int64_t *line_off, int64_t capacity,
                     int64_t *counts, int64_t *err_line, void *workspace, size_t workspace_bytes,
                     void *stream);

/* Pass 2, the tokens of lines [0, n_lines) of pass 1's line_off (n_lines <= its capacity, row0 +
 * n_lines <= n_rows; pow5: device uint64 [1302], the words of dw_pow5_table): table, key_off,
 * key_len, key_i64 at rows row0 .. row0 + n_lines - 1, the undecided entries, counts[1], *err_line
 * and the status bits above. */
int dw_embread_parse(const uint8_t *text, int64_t n_bytes, const int64_t *line_off,
                     int64_t n_lines, int32_t dim, const uint64_t *pow5, float *table,
                     int64_t n_rows, int64_t row0, int64_t *key_off, int64_t *key_len,
                     int64_t *key_i64, int64_t *undecided, int64_t undecided_capacity,
                     int64_t *counts, int64_t *err_line, int32_t *status, void *stream);

/* Raw edges (src, dst int64 [n_edges], ids in [0, 2^id_bits), id_bits <= 60: others set
 * DW_S_BAD_INDEX; weights float64 [n_edges] or NULL) to their canonical form: node_ids int64
 * [<= 2 n_edges] = the distinct ids ascending (a node's rank is its index); edges uint64
 * [<= n_edges] = every undirected pair once, rank(src) << 32 | rank(dst) in the orientation and
 * at the position of its first occurrence; edge_weights float64 = the weight of the pair's last
 * occurrence; counts[0] = nodes, counts[1] = unique edges (device int64 [2]). Self-loops kept. */
int dw_edges_canonical(const int64_t *src, const int64_t *dst, const double *weights,
                       int64_t n_edges, int32_t id_bits, int64_t *node_ids, uint64_t *edges,
                       double *edge_weights, int64_t *counts, int32_t *status, void *workspace,
                       size_t workspace_bytes, void *stream);

/* dw_csr_from_edges for edges that may hold self-loops and carry weights: a self-loop is one
 * entry and one degree (networkx lists it once); edge_weights float64 [n_edges] or NULL goes to
 * both directions (weights float64 [2 n_edges]). row_ptr int64 [n_nodes + 2]; col int32
 * [2 n_edges], of which row_ptr[n_nodes + 1] are written. Endpoints >= n_nodes set DW_S_BAD_CSR
 * and their edge is left out. */
int dw_csr_from_edges_loops(const uint64_t *edges, const double *edge_weights, int64_t n_edges,
                            int64_t n_nodes, int64_t *row_ptr, int32_t *col, double *weights,
                            int32_t *status, void *workspace, size_t workspace_bytes,
                            void *stream);

/* Exact replay walker — bit-exact with DeepWalk.walk / Node2Vec.walk
 * (random_walk_generator.py:61-72 / 94-119) given the uniforms random.random() would return.
 * uniforms: float64[n_walks, L-1], consumed in the reference's order (one per step).
 * out: int32[n_walks, L]. Weighted graphs: weights != NULL (float64, networkx 'weight').
 * Arithmetic follows CPython 3.10 exactly: left-to-right fp64 sum, w *= (1/p), w/sum,
 * itertools.accumulate, total = cum[-1] + 0.0, bisect_right(cum, u*total, 0, deg-1).
 * Unweighted graphs (weights == NULL) reach the same picks without the serial sums: exact
 * class counts give W_i - u*T, decided against a proven rounding bound, with the serial
 * arithmetic only where the bound cannot decide; environment
 * DW_REPLAY_SERIAL=1 forces the serial arithmetic everywhere (a testing aid). */
int dw_walk_replay(const int64_t *row_ptr, const int32_t *col, const int32_t *col_sorted,
                   const double *weights, int64_t n_rows, const int32_t *starts, int64_t n_walks,
                   int32_t walk_length, int32_t method, double p, double q,
                   const double *uniforms, int32_t *out, int32_t *status, void *stream);

/* dw_walk_replay for DeepWalk on an unweighted graph over the edge-inline CSR `edges`
 * (dw_edges_inline_build): the same walks bit for bit (the exact picks of dw_walk_replay, with
 * the serial arithmetic where their bound cannot decide, DW_REPLAY_SERIAL honoured), one
 * dependent 16-B load per step. Replaces random_walk_generator.py:61-72 on unweighted graphs. */
int dw_walk_replay_inline(const int64_t *row_ptr, const int32_t *edges, int64_t n_rows,
                          const int32_t *starts, int64_t n_walks, int32_t walk_length,
                          const double *uniforms, int32_t *out, int32_t *status, void *stream);

/* dw_walk_replay for node2vec on an unweighted graph, over the per-row adjacency hash: the same
 * walks bit for bit. At a step t -> v it probes the shorter of the two lists — N(v)'s classes
 * from t's hash (adj_off / adj_hash), or N(t)'s members' positions in N(v) from v's hash and
 * adj_hpos (dw_adj_hash_positions) — then the exact picks' margin rule, with the serial
 * arithmetic (over col_sorted) where it cannot decide. edge_cn: NULL, or the per-edge class
 * counts of dw_edge_common_counts — a step then classifies N(v) only from its nearer end up to
 * the crossing (same walks). counters: NULL, or uint64[4]
 * (caller-zeroed) += {bytes, hash probes, list entries read, steps} — the realised traffic for
 * the walk roofline (bench.py). Replaces random_walk_generator.py:94-119 on unweighted graphs. */
int dw_walk_replay_indexed(const int64_t *row_ptr, const int32_t *col, const int32_t *col_sorted,
                           const int64_t *adj_off, const int32_t *adj_hash,
                           const int32_t *adj_hpos, const int32_t *hub_idx,
                           const uint32_t *hub_bits, int64_t hub_words,
                           const uint32_t *edge_cn, int64_t n_rows,
                           const int32_t *starts, int64_t n_walks, int32_t walk_length, double p,
                           double q, const double *uniforms, int32_t *out, int32_t *status,
                           uint64_t *counters, void *stream);

/* edge_cn uint32[n_edges] for every directed edge e = (t -> v = col[e]) of row t: bit 31 =
 * [t in N(v)], bits 0-30 = #{x in N(v) : x != t, x in N(t)} — the class counts (x == prev, x a
 * neighbour of prev) of a node2vec step t -> v (random_walk_generator.py:100-108), computed once
 * per graph over the shorter list against the other row: its neighbour bitmap (hub_idx /
 * hub_bits of dw_hub_bitmaps; NULL = none), else its adjacency hash (dw_adj_hash_build); both
 * directions of an undirected edge from one count (the reverse entry through adj_hpos,
 * dw_adj_hash_positions). The graph must be simple (no repeated neighbour in a row). */
int dw_edge_common_counts(const int64_t *row_ptr, const int32_t *col, const int64_t *adj_off,
                          const int32_t *adj_hash, const int32_t *adj_hpos,
                          const int32_t *hub_idx, const uint32_t *hub_bits, int64_t hub_words,
                          int64_t n_rows, int64_t n_edges, uint32_t *edge_cn, void *stream);

/* The node2vec position index, step 1: off int64[n_edges + 1] = exclusive prefix sums of the
 * common-neighbour counts C(e) (edge_cn bits 0-30; off[n_edges] = the index's entry count) and
 * byte_off int64[n_edges + 1] = those of the edges' byte sizes in the compact index: C(e)
 * entries of 2 B (uint16) when the target row col[e] has <= 65536 neighbours, else 4 B
 * (int32), rounded up to 4 B (byte_off[n_edges] = the index's size). tmp == NULL: *tmp_bytes =
 * the scans' scratch size, nothing launched. n_edges < 2^32. */
int dw_n2v_edge_offsets(const int64_t *row_ptr, const int32_t *col, const uint32_t *edge_cn,
                        int64_t n_edges, int64_t *off, int64_t *byte_off, void *tmp,
                        size_t *tmp_bytes, void *stream);

/* The node2vec position index, step 2, for the edges [e_begin, e_end) (random_walk_generator.py:
 * 100-108: at a step t -> v only the 1/p neighbour t and the 1/q neighbours N(t) ∩ N(v) weigh
 * other than 1): writes, at pos + byte_off[e], the positions in N(v) of the C(e) common
 * neighbours of edge e = (t -> v), ascending, as uint16 or int32 (dw_n2v_edge_offsets), and
 * pos_t[e] = the position of t in N(v) or -1. The chunk's entries are off[e_begin] - base ..
 * off[e_end] - base (base = off[e_begin], n_chunk_pos = off[e_end] - base < 2^31); scratch
 * int32[n_chunk_pos] holds the chunk's sorted positions. A caller bounds the scratch by cutting
 * the edges into chunks. Positions come from the shorter list as the counts do (same adjacency
 * index arguments as dw_edge_common_counts); a row whose positions disagree with its count sets
 * DW_S_BAD_CSR in *status. tmp == NULL: *tmp_bytes = the scratch size for n_chunk_pos entries
 * and e_end - e_begin edges. n_edges < 2^31. */
int dw_n2v_edge_index_build(const int64_t *row_ptr, const int32_t *col, const int64_t *adj_off,
                            const int32_t *adj_hash, const int32_t *adj_hpos,
                            const int32_t *hub_idx, const uint32_t *hub_bits, int64_t hub_words,
                            const uint32_t *edge_cn, const int64_t *off, const int64_t *byte_off,
                            int64_t n_rows, int64_t n_edges, int64_t e_begin, int64_t e_end,
                            int64_t base, int64_t n_chunk_pos, uint8_t *pos, int32_t *scratch,
                            int32_t *pos_t, void *tmp, size_t *tmp_bytes, int32_t *status,
                            void *stream);

/* The node2vec position index, step 3: rec int32[n_edges][8], the walker's 32-B edge records
 * {v, deg(v), row_ptr[v] lo, hi, byte_off[e] lo, hi, edge_cn[e], pos_t[e]}. */
int dw_n2v_edge_records(const int64_t *row_ptr, const int32_t *col, const uint32_t *edge_cn,
                        const int64_t *byte_off, const int32_t *pos_t, int64_t n_edges,
                        int32_t *rec, void *stream);

/* ---- deterministic accumulation (SURVEY.md §5 "race detection": run-to-run, eager / graph
 * and 1 / N-rank bit-identical tables) --------------------------------------------------------
 * Registers acc (int64[n_elems], zeroed by the caller) as the accumulator of the float gradient
 * buffer grad: every later SGNS launch whose g_in / g_out is grad adds each gradient term t as
 * round(t * 2^frac) into acc with integer atomics — sums independent of order and of how the
 * terms are split over waves, chunks or ranks — and converts the exact sums back into grad
 * (centre rows after pass 1, output rows in the records gather) unless flags has
 * DW_EXACT_DEFER: then acc keeps the centre sums for the caller to reduce across ranks and
 * convert (dw_fixed_to_float). The records (sorted) output path only; pooled (CBOW) inputs are
 * refused. frac: dw_exact_frac_bits(the launches' grad scale). Host-side registry, keyed by
 * the grad pointer (graph-captured launches keep the accumulator they were captured with). */
#define DW_EXACT_DEFER 1
/* (flags, a centre-table buffer of the one-GPU dense path) the dense Adam converts: pass 1 leaves
 * the centre sums in acc, and dw_adam_dense / dw_adam_dense_to on this buffer read each
 * gradient as fl(acc * 2^-frac) and clear acc (zero_grad) — one streaming pass instead of a
 * conversion pass after pass 1. */
#define DW_EXACT_ADAM 2

/* Row 0 of a lazy Adam history (dw_adam_rows): the box header's tag ("WDBX"). */
#define DW_HIST_BOX_TAG 0x58424457u
int dw_exact_register(const float *grad, int64_t *acc, int64_t n_elems, int32_t frac,
                      int32_t flags);
int dw_exact_unregister(const float *grad);
/* 32 + ceil(-log2 |scale|), clamped to [16, 62]: terms |coef| <= |scale| times entries below
 * 2^19 stay under 2^51, sums under 2^31 fit int64. */
int32_t dw_exact_frac_bits(double scale);
/* grad[i] = (accumulate ? grad[i] : 0) + fl(acc[i] * 2^-frac); acc[i] = 0 (i < n). */
int dw_fixed_to_float(int64_t *acc, float *grad, int64_t n, int32_t frac, int32_t accumulate,
                      void *stream);

/* dw_walk_replay_indexed's walks, bit for bit, over the position index (n2v_rec / n2v_pos of
 * dw_n2v_edge_index_build): one lane per walker, a step reads its edge's 32-B record and
 * binary-searches that edge's positions (log2 C loads), the pick by the margin rule; a pick the
 * margin cannot decide is made by the reference's own fp64 arithmetic (sum, normalise,
 * accumulate, bisect_right) replayed run by run over the position list, O(C + log n) in the
 * walker's lane. counters: NULL, or uint64[5] (caller-zeroed) += {bytes, serial picks, position
 * 2-B units read, steps, the searches' dependent 128-B line moves (a probe in the line of the
 * probe before it not counted)}. Replaces random_walk_generator.py:94-119 on unweighted graphs. */
int dw_walk_replay_positions(const int64_t *row_ptr, const int32_t *n2v_rec,
                             const uint8_t *n2v_pos, int64_t n_rows, const int32_t *starts,
                             int64_t n_walks, int32_t walk_length, double p, double q,
                             const double *uniforms, int32_t *out, int32_t *status,
                             uint64_t *counters, void *stream);

/* Neighbour bitmaps of hub rows for dw_walk_replay_indexed (hub_idx / hub_bits; NULL = none):
 * bits[k * hub_words + (x >> 5)] bit (x & 31) = x in N(hub_rows[k]); hub_words >=
 * ceil(n_rows / 32). A test of a neighbour of v against a hub prev too long for LDS is then one
 * 4-B load instead of a binary search of its sorted list. */
int dw_hub_bitmaps(const int64_t *row_ptr, const int32_t *col, int64_t n_rows,
                   const int32_t *hub_rows, int64_t n_hubs, int64_t hub_words, uint32_t *bits,
                   void *stream);

/* Fast walker (Philox4x32-10 keyed by (seed, walk_id0 + w, step, round/lane)); walks are a pure
 * function of (seed, global walk id), identical for any grid and any number of GPUs.
 *   DeepWalk: one lane per walker; uniform neighbour (unweighted) or alias table (weighted).
 *   node2vec: 8 lanes per walker; rejection rounds of 64 proposals x ~ w(v,x) (Philox counter
 *   field j = 0..63), accepted with alpha(prev,x)/alpha_max under the reference's rule
 *   (x==prev -> 1/p, prev in N(x) -> 1/q, else 1; random_walk_generator.py:101-108); the
 *   lowest accepting j wins — an exact draw from the reference's step law. Proposals are
 *   evaluated 8 at a time in j order; adjacency is tested only where the uniform leaves the
 *   outcome open.
 * prob_thr/alias: NULL for unweighted graphs. col_sorted: required for node2vec (8-ary search
 * of the sorted list). dw_walk_fast_indexed: the same walks (bit-identical) over derived
 * indexes — DeepWalk over the edge-inline CSR `edges` (dw_edges_inline_build; one dependent
 * load per step, walks stored 4 steps per 16-B store), node2vec with its adjacency tests in the
 * per-row hash (adj_off/adj_hash from dw_adj_hash_build; `col` for rows of degree <= 8). */
int dw_walk_fast(const int64_t *row_ptr, const int32_t *col, const int32_t *col_sorted,
                 const uint32_t *prob_thr, const int32_t *alias, int64_t n_rows,
                 const int32_t *starts, int64_t n_walks, int32_t walk_length, int32_t method,
                 double p, double q, uint64_t seed, uint64_t walk_id0, int32_t *out,
                 int32_t *status, void *stream);
int dw_walk_fast_indexed(const int64_t *row_ptr, const int32_t *col, const int32_t *edges,
                         const int64_t *adj_off, const int32_t *adj_hash,
                         const uint32_t *prob_thr, const int32_t *alias, int64_t n_rows,
                         const int32_t *starts, int64_t n_walks, int32_t walk_length,
                         int32_t method, double p, double q, uint64_t seed, uint64_t walk_id0,
                         int32_t *out, int32_t *status, void *stream);

/* dw_walk_fast_indexed's node2vec walks (the same walks, bit for bit) with the walker's realised
 * memory traffic counted, for the walk roofline (bench.py): counters[0..3] (uint64, caller-zeroed,
 * accumulated) += load + store bytes the walkers issued (row_ptr / adj_off pairs, proposal picks,
 * hash buckets or short-list scans, the output), steps, proposal blocks evaluated, adjacency
 * tests. A diagnostic launch: one wave-summed atomic per counter and wave. Replaces no reference
 * interface (the reference has no counters); its walks are Node2Vec.walk's law
 * (random_walk_generator.py:94-119). */
int dw_walk_fast_counted(const int64_t *row_ptr, const int32_t *col, const int64_t *adj_off,
                         const int32_t *adj_hash, const uint32_t *prob_thr, const int32_t *alias,
                         int64_t n_rows, const int32_t *starts, int64_t n_walks,
                         int32_t walk_length, double p, double q, uint64_t seed,
                         uint64_t walk_id0, int32_t *out, int32_t *status,
                         uint64_t *counters, void *stream);

/* node2vec with Philox draws over the per-edge position index (n2v_rec / n2v_pos from
 * dw_n2v_edge_index_build): one lane per walker, one 32-B edge record and log2 C dependent 2-B
 * (4-B for a hub target's list) position loads per step, no rejection rounds. The law is Node2Vec.walk's
 * (random_walk_generator.py:94-119, the reference's inverted q rule): step 1 picks
 * bounded32(r.x, deg) (:97, prev None), later steps the first neighbour i whose exact prefix
 * weight W_i = a_i/p + b_i + c_i/q exceeds U*T, U = 53 bits of (r.x, r.y), with the fp64
 * expressions of the exact replay's pick; Philox counter (walk id lo, hi, step << 8, 'NP').
 * Unweighted graphs (the index has no weights). counters: NULL, or uint64[4] += {load + store
 * bytes, steps, the searches' dependent 128-B line moves, position 2-B units read}. Reads
 * walk_id0 from a bound dw_step_scalars block. */
int dw_walk_fast_positions(const int64_t *row_ptr, const int32_t *n2v_rec, const uint8_t *n2v_pos,
                           int64_t n_rows, const int32_t *starts, int64_t n_walks,
                           int32_t walk_length, double p, double q, uint64_t seed,
                           uint64_t walk_id0, int32_t *out, int32_t *status, uint64_t *counters,
                           void *stream);

/* Edge-inline CSR for DeepWalk in dw_walk_fast_indexed: edges int32[nnz][4], entry e of row u =
 * {x = col[e], deg(x), row_ptr[x] low 32 bits, row_ptr[x] high 32 bits}. The pick of the next
 * node then also yields its row: one dependent load per walk step instead of two — the
 * `get_node_neighbors` + `random.choices` step of DeepWalk.walk (random_walk_generator.py:41-42,
 * 61-72) as one 16-B read. */
int dw_edges_inline_build(const int64_t *row_ptr, const int32_t *col, int64_t n_rows, int64_t nnz,
                          int32_t *edges, void *stream);

/* ---- SGNS (skip-gram negative sampling) ---------------------------------------------------------- */

/* Fused SGNS over walks: W2VCollateFunctional sg windows (torch_dataset.py:300-309) +
 * generate_noise_batch (sampling.py:7-21) + SkipGram.forward x2 (model.py:79-91) +
 * NegativeSamplingLoss (loss.py:14-22) + the closed-form backward of all of it
 * (clamp(sigmoid,1e-6) zero-gradient mask), accumulated into dense gradient tables.
 *   walks: int32[n_walks, L] vocabulary ids; centres are positions R..L-R-1 of every walk,
 *          centre b = w*(L-2R) + (i-R); contexts left-then-right.
 *   noise: int64[B', 2R, K] replayed negatives, or NULL = draw uniform [0,V) on device with
 *          Philox keyed by (seed, noise_offset + b, j*K + k).
 *   w_in/w_out: float32[V, d] (in/out embedding tables, row-major);
 *   g_in/g_out: float32[V, d] gradients, ACCUMULATED (+=);
 *   grad_scale: d(loss)/d(term) = 1/M, M = total centres*2R of the (global) batch.
 *   loss_acc: float64[4] accumulated (+=): sum positive-loss, sum negative-loss (summed over K),
 *             count(sigmoid(s)>=0.5), count(sigmoid(t)>=0.5)  (trainer.py:145-150).
 *   workspace: NULL -> output-table gradients scattered with float atomics;
 *              non-NULL (>= dw_sgns_walks_workspace_bytes) -> atomic-free output-table path: one
 *              {row, centre, coef} record per output row — with walk aggregation (below) one
 *              per negative and one per walk position — radix-sorted by row, then summed per
 *              row from gathered centre rows (stable order: g_out is reproducible run to run
 *              except at rows straddling two 512-record chunks). The centre-table gradient is
 *              one float-atomic row per centre in both modes. */
int dw_sgns_walks(const int32_t *walks, int64_t n_walks, int32_t walk_length,
                  int32_t context_radius, int32_t neg_samples, int64_t vocab_size, int32_t dim,
                  const float *w_in, const float *w_out, float *g_in, float *g_out,
                  const int64_t *noise, uint64_t seed, uint64_t noise_offset, float grad_scale,
                  double *loss_acc, int32_t *status, void *workspace, size_t workspace_bytes,
                  void *stream);

/* Two-phase form of dw_sgns_walks (same arguments, plus phase): phase 1 runs pass 1 — the
 * centre-table gradient g_in, the loss sums and the output-row records in the workspace —
 * and phase 2 sorts the records and accumulates g_out. A phase-2 call must follow the phase-1
 * call with identical arguments on the same stream; between the two, g_in is final and may be
 * read (the multi-GPU exchange starts its reduce-scatter there, overlapping phase 2). phase 0
 * is dw_sgns_walks. In atomic mode (workspace NULL) phase 1 does everything. */
int dw_sgns_walks_phase(int32_t phase, const int32_t *walks, int64_t n_walks,
                        int32_t walk_length, int32_t context_radius, int32_t neg_samples,
                        int64_t vocab_size, int32_t dim, const float *w_in, const float *w_out,
                        float *g_in, float *g_out, const int64_t *noise, uint64_t seed,
                        uint64_t noise_offset, float grad_scale, double *loss_acc,
                        int32_t *status, void *workspace, size_t workspace_bytes,
                        void *stream);

/* Phase 2 of dw_sgns_walks_phase in row pieces (N > 1: ShardedTables pipelines each piece's
 * output-table exchange behind the next piece's gather). Piece p covers output rows
 * [p * piece_rows, (p+1) * piece_rows); n_pieces * piece_rows >= vocab_size, n_pieces <= 1024.
 *   piece == -1: the records sort of the preceding phase-1 call and the record bounds of the
 *                pieces (in the workspace);
 *   piece in [0, n_pieces): g_out += the gradient of piece p's rows (complete when it returns
 *                in stream order; other rows untouched).
 * Calls -1, 0, ..., n_pieces-1 in order equal phase 2. Arguments as dw_sgns_walks_phase, same
 * workspace (a workspace holds one sorted batch at a time). */
int dw_sgns_walks_phase2_piece(int32_t piece, int32_t n_pieces, int64_t piece_rows,
                               const int32_t *walks, int64_t n_walks, int32_t walk_length,
                               int32_t context_radius, int32_t neg_samples, int64_t vocab_size,
                               int32_t dim, const float *w_in, float *g_out, int32_t *status,
                               void *workspace, size_t workspace_bytes, void *stream);

/* Phase 2 of dw_sgns_walks_phase fused with the output table's dense Adam step (one device):
 * the same records sort + gather, but every out row is updated in place with torch.optim.Adam
 * (single-tensor semantics, the scalars of dw_adam_dense) using its complete gradient —
 * rows wholly inside one gather chunk straight from registers, the rest (chunk-boundary rows,
 * rows without records: g = 0) from g_out. Equals phase 2 followed by dw_adam_dense(w_out,
 * g_out, m_out, v_out, ..., zero_grad = 1); g_out must be zero on entry and is left zero;
 * row_flags: vocab_size bytes, zero on entry, left zero. Arguments as dw_sgns_walks_phase
 * (g_in, noise, seed, loss_acc are not used by phase 2). */
int dw_sgns_walks_phase2_adam(const int32_t *walks, int64_t n_walks, int32_t walk_length,
                              int32_t context_radius, int32_t neg_samples, int64_t vocab_size,
                              int32_t dim, const float *w_in, float *w_out, float *g_out,
                              float *m_out, float *v_out, uint8_t *row_flags,
                              float one_minus_beta1, float beta2, float one_minus_beta2,
                              float bias_correction2_sqrt, float neg_step_size, float eps,
                              float weight_decay, int32_t *status, void *workspace,
                              size_t workspace_bytes, void *stream);

/* Owner-computes form of the walks SGNS step for N > 1 (ShardedTables(mode='owner'), bench.py).
 * The output ("context") table is sharded by row owner: rank `owner` of `n_owners` holds only
 * rows o with o % n_owners == owner, as local row o / n_owners of w_out_local
 * (float32[local_rows, d], local_rows * n_owners >= vocab_size). Every rank passes the WHOLE
 * global batch of walks (walks are keyed by global id, so each rank forms them itself) and the
 * full, replicated in table; it computes only the output slots it owns, so no output-table
 * gradient or parameter ever crosses ranks. Replaces the reference's single-device step
 * (trainer.py:131-152 + the dense Adam of config_parser/core.py:43-53) at N > 1; summed over the
 * owners, the work is exactly dw_sgns_walks_phase's.
 * pass 1: g_in += the centre-table gradient of the owned slots (a PARTIAL sum: the caller
 *         reduces it across ranks), loss_acc += their loss terms, records kept in the
 *         workspace (>= dw_sgns_owner_workspace_bytes(n_walks*(L-2R), 2R, K, V, local_rows)),
 *         packed in a fixed order (deterministic).
 *         Needs dim a multiple of 64 (<= 512) and 2R(1+K) <= 64 (else DW_E_UNSUPPORTED).
 * pass 2: sorts the records by local row and accumulates the slice's gradient: with m_out
 *         non-NULL, the slice's torch.optim.Adam step is fused in exactly as in
 *         dw_sgns_walks_phase2_adam (g_out_local zero on entry and left zero, row_flags
 *         local_rows bytes); with m_out NULL, g_out_local += the gradient. With n_records
 *         non-NULL it reads the record count back to the host (ONE synchronisation of
 *         `stream`) into *n_records and sorts exactly that many; with n_records NULL there is
 *         no synchronisation: the sort runs over the bound n_walks*(L-2R)*2R(1+K) with the
 *         tail padded past every row and the gather limited on the device — the choice for
 *         n_owners = 1, where every slot is kept and the bound is the count. Same walk sizes
 *         and workspace as the pass-1 call. */
int dw_sgns_owner_workspace_bytes(int64_t n_centres, int32_t n_ctx, int32_t neg_samples,
                                  int64_t vocab_size, int64_t local_rows, size_t *bytes);
/* The owner form's centre order for a batch ahead of pass 1 (pass 1 with order_ready = 1 uses
 * it instead of building its own): the centres sorted by node (stable). touched (optional,
 * uint32[n_walks*(L-2R)]) receives the batch's distinct centre nodes in increasing order and
 * *n_touched (device int64) their count — the rows a step reads and updates in the in table
 * (OwnerLazyTables). Same workspace as the pass-1 / pass-2 calls that follow.
 * dw_sgns_owner_pass1's order_ready is a bit set: 1 = this order is ready (else pass 1 builds
 * it); 2 = the records are placed (dw_sgns_owner_out_catch_up ran with flags & 1 on this batch
 * and workspace): pass 1 writes each record straight into its row's segment, and
 * dw_sgns_owner_pass2_lazy (flags & 1) gathers them without a sort; 4 (with 2) = coefficients in:
 * dw_sgns_owner_out_rows already formed every record's coefficient and left each row it stepped
 * pending, its pre-step values in w_out_local — pass 1 forms the centre gradient alone (no loss
 * sums, no records written; loss_acc may be NULL); 8 (with 4) = the centres in walk order (no
 * node order is built or read: one atomic row per centre occurrence). */
int dw_sgns_owner_prepare(const int32_t *walks, int64_t n_walks, int32_t walk_length,
                          int32_t context_radius, int32_t neg_samples, int64_t vocab_size,
                          int64_t local_rows, uint32_t *touched, int64_t *n_touched,
                          void *workspace, size_t workspace_bytes, void *stream);
int dw_sgns_owner_pass1(const int32_t *walks, int64_t n_walks, int32_t walk_length,
                        int32_t context_radius, int32_t neg_samples, int64_t vocab_size,
                        int32_t dim, int32_t owner, int32_t n_owners, int64_t local_rows,
                        int32_t order_ready, const float *w_in, const float *w_out_local,
                        float *g_in,
                        const int64_t *noise, uint64_t seed, uint64_t noise_offset,
                        float grad_scale, double *loss_acc, int32_t *status, void *workspace,
                        size_t workspace_bytes, void *stream);
int dw_sgns_owner_pass2(int64_t n_walks, int32_t walk_length, int32_t context_radius,
                        int32_t neg_samples, int64_t local_rows, int32_t dim, const float *w_in,
                        float *w_out_local, float *g_out_local, float *m_out, float *v_out,
                        uint8_t *row_flags, float one_minus_beta1, float beta2,
                        float one_minus_beta2, float bias_correction2_sqrt, float neg_step_size,
                        float eps, float weight_decay, int32_t *status, void *workspace,
                        size_t workspace_bytes, int64_t *n_records, void *stream);

/* The lazy out slice's catch-up, before dw_sgns_owner_pass1 of the same batch: every owned
 * output row a slot references (contexts from the walks, negatives as pass 1 draws them) is
 * brought current to step - 1 (its deferred g = 0 steps replayed, hist as above), so pass 1 reads
 * the rows the dense update holds. claim int32 [local_rows] (zero-initialised, never reset): a
 * row is listed once per step, claimed via atomicMax(claim[row], step), when its last claim is
 * older than step - 1; rows_buf uint32 [min(local_rows, B' * 2R(1+K))] and n_rows (int64,
 * device) receive the list, which is then replayed. flags (a bit set):
 *   1 = place the records: counts uint32 [local_rows + 1] (zero-initialised; the placement
 *       scan clears it once read, so it is zero between steps) counts every row's slots, each
 *       slot's rank among them and the exclusive scan of the counts go to `workspace` (the owner
 *       form's, dw_sgns_owner_workspace_bytes), for dw_sgns_owner_pass1 (order_ready | 2) and
 *       dw_sgns_owner_pass2_lazy (flags | 1, the same counts): the records land grouped by row,
 *       no sort (the order of one row's records is the order the atomics resolved);
 *   2 = replay p only: m, v and last_step stay behind, and dw_sgns_owner_pass2_lazy (flags | 2)
 *       replays m and v (a multiply each per step) before the step — valid while every step has
 *       weight_decay 0;
 *   4 (with 1) = the rows-major step follows (dw_sgns_owner_out_rows): only the ranks and the
 *       scan — no claim, no list, no replay — then every slot is placed (its row and slot id in
 *       the workspace's records); claim and rows_buf are not touched.
 * 2R(1+K) <= 64, dim <= 512. */
int dw_sgns_owner_out_catch_up(const int32_t *walks, int64_t n_walks, int32_t walk_length,
                               int32_t context_radius, int32_t neg_samples, int64_t vocab_size,
                               int32_t dim, int32_t owner, int32_t n_owners, int64_t local_rows,
                               const int64_t *noise, uint64_t seed, uint64_t noise_offset,
                               float *w_out_local, float *m_out, float *v_out,
                               int32_t *last_step, int32_t *claim, uint32_t *counts,
                               uint32_t *rows_buf, int64_t *n_rows, const float *hist,
                               int32_t step, int32_t flags, int32_t *status, void *workspace,
                               size_t workspace_bytes, void *stream);

/* dw_sgns_owner_pass2 with the out slice's Adam kept LAZY and exact (OwnerLazyTables, small
 * batches): a row no record touched is not read or written; its deferred g = 0 steps are
 * replayed (scalars hist[t], fp32 [steps][8] as for dw_adam_rows) right before its next update,
 * through the same adam_elem, so the slice equals the dense update bit for bit once flushed
 * (dw_adam_rows with rows = NULL). last_step int32 [local_rows]: the step each row is current
 * to; step: this step (>= 1). torch.optim.Adam semantics (config_parser/core.py:43-53).
 * flags: 1 = the records were placed (see dw_sgns_owner_out_catch_up; n_records NULL; counts:
 * its row counts, already cleared by its scan), 2 = the catch-up replayed p only (m, v are
 * replayed here), 4 = every step so far had the same betas (those replays use this step's). */
int dw_sgns_owner_pass2_lazy(int64_t n_walks, int32_t walk_length, int32_t context_radius,
                             int32_t neg_samples, int64_t local_rows, int32_t dim,
                             const float *w_in, float *w_out_local, float *g_out_local,
                             float *m_out, float *v_out, int32_t *last_step, const float *hist,
                             int32_t step, int32_t flags, uint32_t *counts, int32_t *status,
                             void *workspace, size_t workspace_bytes, int64_t *n_records,
                             void *stream);

/* The distinct centre nodes of a batch (the in rows one step touches), UNSORTED, for the lazy
 * in-table update on one rank (dw_sgns_owner_prepare gives them sorted, the order every rank
 * agrees on when N > 1): claim int32 [vocab_size] (zero-initialised, kept across steps) gets
 * claim[node] = step and the first claimer lists the node in touched (uint32 [>= B']);
 * n_touched (int64, device) their count. fresh / n_fresh (NULL = not wanted): the listed
 * nodes whose claim was below step - 1 — not centres of the step before, so nothing of that
 * step writes their rows (the pipelined step catches them up while step - 1 still runs). Reads
 * step from a bound dw_step_scalars block (relative form). flags: 0, or 1 = the counters are
 * already zero (not reset here: a caller that clears many steps' counters at once). Replaces
 * nothing in the reference (its optimizer steps every row). */
int dw_sgns_owner_touch_claim(const int32_t *walks, int64_t n_walks, int32_t walk_length,
                              int32_t context_radius, int64_t vocab_size, int32_t *claim,
                              int32_t step, uint32_t *touched, int64_t *n_touched,
                              uint32_t *fresh, int64_t *n_fresh, int32_t flags, void *stream);

/* The rows-major lazy out step (OwnerLazyTables, one device; after dw_sgns_owner_out_catch_up
 * with flags 1 | 4 on the same batch and workspace, before dw_sgns_owner_pass1 with order_ready
 * 1 | 2 | 4): each owned out row the batch touches is read once and written once — its deferred
 * g = 0 steps replayed (hist, as for dw_adam_rows), the logits of its records against their
 * centre rows, the coefficients and loss sums (loss_acc float64[4] as for dw_sgns_walks), its
 * gradient and the Adam step `step` — the same arithmetic as the catch-up / pass 1 /
 * dw_sgns_owner_pass2_lazy sequence. Leaves each record's coefficient in the placed records
 * and every row it steps PENDING for dw_sgns_owner_pass1's centre gradient: exp_avg and
 * exp_avg_sq at `step`, the parameter row still at step - 1 (what the centre gradient reads),
 * pending[row] = 1 (uint8 [local_rows], zero-initialised by the caller). The parameter half of
 * a pending row's step (torch Adam's p update from its m and v, the same operations) is applied
 * when the row is next replayed — by the next rows-major step, or by dw_adam_rows given the same
 * `pending` (the flush before the table is read whole). counts: the catch-up's (already cleared
 * by its placement scan; not written here). dim in {64, 128, 256, 512}, 2R(1+K) <= 64; the
 * deterministic mode (g_out registered) sums each row's terms as integers. */
int dw_sgns_owner_out_rows(const int32_t *walks, int64_t n_walks, int32_t walk_length,
                           int32_t context_radius, int32_t neg_samples, int64_t vocab_size,
                           int32_t dim, int32_t owner, int32_t n_owners, int64_t local_rows,
                           const int64_t *noise, uint64_t seed, uint64_t noise_offset,
                           float grad_scale, const float *w_in, float *w_out_local,
                           float *g_out_local, float *m_out, float *v_out, int32_t *last_step,
                           uint32_t *counts, uint8_t *pending, const float *hist,
                           int32_t step, double *loss_acc, int32_t *status,
                           void *workspace, size_t workspace_bytes, void *stream);

/* Same computation over explicit pairs (the reference's collate output):
 * inputs int64[B], targets int64[B, C], noise int64[B, C, K] or NULL (Philox as above). */
int dw_sgns_pairs(const int64_t *inputs, const int64_t *targets, int64_t batch, int32_t n_ctx,
                  int32_t neg_samples, int64_t vocab_size, int32_t dim,
                  const float *w_in, const float *w_out, float *g_in, float *g_out,
                  const int64_t *noise, uint64_t seed, uint64_t noise_offset, float grad_scale,
                  double *loss_acc, int32_t *status, void *workspace, size_t workspace_bytes,
                  void *stream);

/* Pooled-input (CBOW) form of dw_sgns_pairs (model.py:94-110 CBOW.forward + loss.py:14-22 +
 * trainer.py:131-152): the input vector of sample b is the mean of w_in rows inputs[b, 0..n_in)
 * (torch.mean over dim 1); targets int64 [batch, n_ctx] are the positive output rows and the
 * noise [batch, n_ctx, neg_samples] (or device Philox, NULL) the negatives. Each of the n_in
 * input rows receives 1/n_in of the input-vector gradient (mean backward). n_in = 1 computes
 * what dw_sgns_pairs computes. Always the atomic output-table scatter (text-corpus batches). */
int dw_sgns_pooled_pairs(const int64_t *inputs, int32_t n_in, const int64_t *targets,
                         int64_t batch, int32_t n_ctx, int32_t neg_samples, int64_t vocab_size,
                         int32_t dim, const float *w_in, const float *w_out, float *g_in,
                         float *g_out, const int64_t *noise, uint64_t seed,
                         uint64_t noise_offset, float grad_scale, double *loss_acc,
                         int32_t *status, void *stream);

/* Shared-negatives SGNS over walks (a documented DEPARTURE from the reference):
 * the L - 2R centres of walk w share the n_shared = S ids shared_ids[w, 0..S) as their negatives
 * instead of drawing 2R x K each; the contexts are the walk's own nodes as in dw_sgns_walks. With
 * lambda = 2R * K / S (K = neg_samples stays the nominal negatives per pair, so the loss keeps
 * its expectation and scale):
 *   loss_acc[0] += sum_i sum_ctx -log max(sigmoid(h_i . o_ctx), 1e-6),  [2] += count(sigmoid >= .5)
 *   loss_acc[1] += lambda * sum_i sum_s -log max(sigmoid(-h_i . o_s), 1e-6),
 *   loss_acc[3] += lambda * count(sigmoid(h_i . o_s) >= .5)
 * and g_in / g_out += the closed-form gradient of exactly that loss times grad_scale (positive
 * coefficient (sigmoid - 1) * scale, negative (1 - sigmoid(-x)) * lambda * scale, 0 where the
 * clamp cuts). An id that repeats among a walk's S ids or equals a walk node is its own term.
 * Ids outside [0, V) set DW_S_BAD_INDEX and drop their terms (dw_sgns_walks's convention).
 *   shared_ids: int64[n_walks, n_shared], e.g. dw_sgns_noise(batch = n_walks, n_ctx = 1,
 *               neg_samples = S) or dw_sgns_noise_alias.
 * One block per walk: logits and both gradients are 32x32 f32-MFMA products, every gradient row
 * leaves as float atomics; no workspace. Supported: dim in {64, 128, 256}; n_shared a multiple of
 * 32 in [32, 128]; 2R + 1 <= walk_length <= 128; vocab_size < 2^31; anything else is
 * DW_E_INVALID_ARG (checked before any device call). */
int dw_sgns_walks_shared(const int32_t *walks, int64_t n_walks, int32_t walk_length,
                         int32_t context_radius, int32_t neg_samples, int32_t n_shared,
                         int64_t vocab_size, int32_t dim, const float *w_in, const float *w_out,
                         float *g_in, float *g_out, const int64_t *shared_ids, float grad_scale,
                         double *loss_acc, int32_t *status, void *stream);

/* The device negatives dw_sgns_* draw when noise == NULL, written out: noise[(b*n_ctx + j)*K + k]
 * for b < batch (centre counter noise_offset + b). Replaces generate_noise_batch
 * (utils/sampling.py:7-21) where the ids must exist before the step (max_norm renormalisation).*/
int dw_sgns_noise(int64_t batch, int32_t n_ctx, int32_t neg_samples, int64_t vocab_size,
                  uint64_t seed, uint64_t noise_offset, int64_t *noise, void *stream);

/* ---- unigram^power negatives (noise='unigram') ---------------------------------------------
 * A documented DEPARTURE from the reference's law: generate_noise_batch (utils/sampling.py:7-21)
 * draws negatives uniformly over [0, V); word2vec.c, gensim and the node2vec reference code draw
 * them from the unigram law raised to 0.75. These two entry points draw from any weight vector
 * over the vocabulary (the caller raises its counts or degrees to the power itself).
 *
 * dw_noise_alias_build (HOST, no device work; weights and table are HOST buffers): the Vose
 * alias table of weights[0..V) in float64 — scaled weight w[i] * V / sum, the small list
 * growing from the front of one stack, the large list from its back, both popping from the top
 * (dw_alias_build's discipline). table[i] = {alias id << 32 | prob_thr}, prob_thr =
 * floor(p * 2^32) with 0xFFFFFFFF = always keep i. An id of weight 0 is never drawn: its
 * prob_thr is 0, also where rounding leaves it on the small stack after the large stack ran out
 * (its alias is then the first id of the largest weight). DW_E_INVALID_ARG for V < 1,
 * V >= 2^31, a negative or non-finite weight, or a sum that is not positive and finite.
 *
 * dw_sgns_noise_alias (table: DEVICE uint64[vocab_size]): noise[(b*n_ctx + j)*K + k] for
 * b < batch from the Philox call of dw_sgns_noise — counter (g lo, g hi, n >> 1, 'SG') with
 * g = noise_offset + b, n = j*K + k, words (x, y) = (lo, hi) for even n and (z, w) for odd n.
 * With T = hi*V + ((lo*V) >> 32): slot i = T >> 32 (dw_sgns_noise's id), f = T's low word
 * (the fraction of r64 * V / 2^64), id = i when prob_thr(i) is 0xFFFFFFFF or f < prob_thr(i),
 * else alias(i). Equal weights give dw_sgns_noise's output bit for bit. With a dw_step_scalars
 * block bound, noise_offset is read from it (a captured step draws each replay's negatives). */
int dw_noise_alias_build(const double *weights, int64_t V, uint64_t *table);
int dw_sgns_noise_alias(int64_t batch, int32_t n_ctx, int32_t neg_samples, int64_t vocab_size,
                        const uint64_t *table, uint64_t seed, uint64_t noise_offset,
                        int64_t *noise, void *stream);

/* ---- link prediction on the device (shallow_encoders/graph/linkpred.py) ---------------------
 * The reference's link-prediction protocol (tools/graph_model_downstream_classification.py:
 * 170-200, 241-299) with everything that scales with the edge count on the device.
 *
 * dw_negative_edges: pairs int64[n, 2] of non-adjacent nodes under the reference's law
 * (tools/graph_model_downstream_classification.py:170-200: u uniform over the nodes, v uniform
 * over the nodes not adjacent to u, u itself allowed), without rejection. The nodes are rows
 * first_node .. n_rows - 1 (first_node = 1 in the package: row 0 is <unk>), Nn = n_rows -
 * first_node. Sample i, g = offset + i, draws philox<10>({lo(g), hi(g), 0, 'LP' << 16}, seed lo,
 * seed hi): u = first_node + bounded64(x, y, Nn), m = Nn - deg(u), k = bounded64(z, w, m), and
 * with c u's row of col_sorted (dw_csr_sort_copy) v = first_node + k + j, j the smallest index
 * with c[j] - first_node - j > k (deg(u) when there is none): the k-th non-neighbour by rank, one
 * binary search. Needs distinct neighbours per row (dw_csr_check_simple) and no neighbour below
 * first_node; m <= 0 sets DW_S_BAD_CSR and writes (u, u). */
int dw_negative_edges(const int64_t *row_ptr, const int32_t *col_sorted, int64_t n_rows,
                      int64_t first_node, int64_t n, uint64_t seed, uint64_t offset,
                      int64_t *pairs, int32_t *status, void *stream);

/* out float[n, dim] = op(table[pairs[i, 0]], table[pairs[i, 1]]) — edge_operators.edge_embeddings
 * (shallow_encoders/graph/edge_operators.py:5-55) on float32 rows: op 0 average (a + b) * 0.5f,
 * 1 hadamard a * b, 2 weighted_l1 fabsf(a - b), 3 weighted_l2 (a - b) * (a - b), each in fp32 in
 * exactly that operation order (no contraction). 1 <= dim <= 512; 16-B accesses when dim % 4 == 0
 * and table and out are 16-B aligned. An id outside [0, vocab_size) sets DW_S_BAD_INDEX and its
 * row is written as zeros (nothing out of range is read). */
int dw_edge_features(const float *table, int64_t vocab_size, int32_t dim, int32_t op,
                     const int64_t *pairs, int64_t n, float *out, int32_t *status, void *stream);

/* One pass of a logistic regression over n labelled pairs, no feature stored — the loss,
 * gradient and accuracy sklearn's LogisticRegression.fit / .score compute from the feature
 * matrix of tools/graph_model_downstream_classification.py:241-299. coef double[dim + 1]
 * (weights, then intercept; DEVICE memory), labels uint8[n] (non-zero = positive). Per sample:
 * x = op(a, b) in fp32 as dw_edge_features; in float64 z = w . x + b0,
 * loss = log1p(exp(-|z|)) + max(z, 0) - y z, r = 1 / (1 + exp(-z)) - y. out double[dim + 3]:
 * [0, dim) = sum r x, [dim] = sum r, [dim + 1] = sum loss, [dim + 2] = #{(z > 0) == y}. All sums
 * float64 and reproducible bit for bit: per-block partial rows in the workspace
 * (>= dw_edge_logreg_workspace_bytes(n, dim)) added in block order by a second kernel, a grid
 * that depends on (n, dim) and the table's 16-B alignment only, no float atomics. An id outside
 * [0, vocab_size) sets DW_S_BAD_INDEX and counts as x = 0. n = 0 writes nothing. */
int dw_edge_logreg_workspace_bytes(int64_t n, int32_t dim, size_t *bytes);
int dw_edge_logreg(const float *table, int64_t vocab_size, int32_t dim, int32_t op,
                   const int64_t *pairs, const uint8_t *labels, int64_t n, const double *coef,
                   double *out, void *workspace, size_t workspace_bytes, int32_t *status,
                   void *stream);

/* z_out double[n]: the score of every pair, z = w . x + b0 with x = op(a, b) in fp32 exactly as
 * dw_edge_features computes it and everything after it in float64, as dw_edge_logreg (the same
 * gather: a group of lanes owns a pair, several pairs in flight per group; no atomic and no
 * reduction across pairs, so reruns are bit-identical). coef double[dim + 1] in DEVICE memory, or
 * NULL for unit weights and a zero intercept: with op 1 (hadamard) that is the plain dot product
 * of the two rows. 1 <= dim <= 512; 16-B loads when dim % 4 == 0 and table is 16-B aligned. An
 * id outside [0, vocab_size) sets DW_S_BAD_INDEX and its pair scores as x = 0. */
int dw_edge_scores(const float *table, int64_t vocab_size, int32_t dim, int32_t op,
                   const int64_t *pairs, int64_t n, const double *coef, double *z_out,
                   int32_t *status, void *stream);

/* Exact ROC-AUC counts of n scores (double) with labels uint8[n] (non-zero = positive).
 * out int64[3] (DEVICE memory): [0] = U2 = sum over positives i of 2 #{negatives j: s_j < s_i} +
 * #{negatives j: s_j = s_i}, [1] = n_pos, [2] = n_neg; AUC = U2 / (2 n_pos n_neg), divided by the
 * host (the tie-aware Mann-Whitney statistic, sklearn's roc_auc_score up to that division).
 * Integer sums only: bit-identical on every run. -0.0 ties with +0.0, +-inf are ordinary values,
 * a NaN sets DW_S_NAN_SCORE and leaves out unspecified. n < 2^31; n = 0 writes zeros. workspace:
 * >= dw_roc_auc_workspace_bytes(n) bytes, 256-B aligned. */
int dw_roc_auc_workspace_bytes(int64_t n, size_t *bytes);
int dw_roc_auc(const double *scores, const uint8_t *labels, int64_t n, int64_t *out,
               int32_t *status, void *workspace, size_t workspace_bytes, void *stream);

/* ---- held-out edge split (shallow_encoders/graph/holdout.py) ----------------
 * Hides edges of a simple undirected CSR (distinct neighbours per row, both directed entries of
 * every edge, a self-loop one entry, no neighbour on row 0) so that every node keeps one. With
 * mix64 splitmix64's finaliser (z = x + 0x9E3779B97F4A7C15; z = (z ^ z >> 30) *
 * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31), the priority of edge
 * {u, v}, u < v, is mix64(((u << 32) | v) ^ mix64(seed)): distinct for distinct edges. Self-loops
 * are never held and protect nothing. Every node protects its non-loop edge of smallest
 * priority; the candidates are the non-loop edges neither endpoint protects; held are the n_hold
 * candidates of smallest priority.
 *
 * dw_edge_holdout_count: counts int64[2] (DEVICE memory) = {E_nl, the non-loop edges;
 * n_candidates}. The host reads them, fixes n_hold <= n_candidates and calls dw_edge_holdout
 * with the SAME workspace, untouched in between (it holds the per-node minima and the
 * candidates' priorities).
 * dw_edge_holdout: row_ptr_out int64[n_rows + 1], col_out int32[nnz - 2 n_hold] and weights_out
 * (when weights is not NULL) = the CSR without both entries of every held edge, each row
 * compacted in order; held int64[n_hold, 2] = the held edges (u, v), u < v, in the order of
 * their col > row entries in the input. n_hold = 0 copies the graph.
 * A neighbour on row 0 or outside [1, n_rows) sets DW_S_BAD_CSR (the entry is kept, nothing out
 * of range is read); counts that do not add up to nnz - 2 n_hold and n_hold set DW_S_DUP_NEIGHBOR
 * (a repeated neighbour repeats a priority) and nothing is written out of range. n_rows and nnz
 * below 2^31. workspace: >= dw_edge_holdout_workspace_bytes(n_rows, nnz) bytes, 256-B aligned.
 * Integer atomics, a sort of distinct keys and a scan: reruns are bit-identical. */
int dw_edge_holdout_workspace_bytes(int64_t n_rows, int64_t nnz, size_t *bytes);
int dw_edge_holdout_count(const int64_t *row_ptr, const int32_t *col, int64_t n_rows, int64_t nnz,
                          uint64_t seed, int64_t *counts, int32_t *status, void *workspace,
                          size_t workspace_bytes, void *stream);
int dw_edge_holdout(const int64_t *row_ptr, const int32_t *col, const double *weights,
                    int64_t n_rows, int64_t nnz, uint64_t seed, int64_t n_candidates,
                    int64_t n_hold, int64_t *row_ptr_out, int32_t *col_out, double *weights_out,
                    int64_t *held, int32_t *status, void *workspace, size_t workspace_bytes,
                    void *stream);

/* ---- minimum spanning forest, connected components, the split that keeps them ---------------
 * dw_edge_forest: the minimum spanning forest of the non-loop edges of the same simple
 * undirected CSR under the priorities above (distinct, so the forest is unique), by Boruvka
 * rounds over the entries: forest uint8[nnz] = 1 on both directed entries of every forest edge,
 * else 0; component int32[n_rows] = the smallest row of the row's connected component (a row
 * without a non-loop edge, row 0 included, is its own); counts int64[4] (DEVICE memory) = {E_nl,
 * n_forest, the components that hold a non-loop edge, the rounds that joined components}, so
 * n_forest = (rows with a non-loop edge) - counts[2]. ceil(log2 n_rows) rounds always suffice
 * and that many are launched, asynchronously; the rounds after the last that joined anything
 * return at once. Should the last one still join components, DW_S_FOREST_ROUNDS is set and the
 * outputs are not a forest. A neighbour out of range sets DW_S_BAD_CSR, as does an entry x -> y
 * whose mate y -> x is missing when the forest would need it; neither is used as an index.
 * workspace: >= dw_edge_forest_workspace_bytes(n_rows, nnz) bytes, 256-B aligned. Integer
 * atomics only: reruns are bit-identical.
 *
 * dw_edge_holdout_count_protected / dw_edge_holdout_protected: dw_edge_holdout_count /
 * dw_edge_holdout with the rule "every node protects its edge of smallest priority" replaced by
 * protect uint8[nnz] (never NULL, nnz = 0 included): a non-loop edge is a candidate when its
 * entries' flags are 0 (both entries of an edge must agree). With dw_edge_forest's flags the residual graph keeps every connected
 * component of the input and no bridge is held. Everything else is as above. */
int dw_edge_forest_workspace_bytes(int64_t n_rows, int64_t nnz, size_t *bytes);
int dw_edge_forest(const int64_t *row_ptr, const int32_t *col, int64_t n_rows, int64_t nnz,
                   uint64_t seed, uint8_t *forest, int32_t *component, int64_t *counts,
                   int32_t *status, void *workspace, size_t workspace_bytes, void *stream);
int dw_edge_holdout_count_protected(const int64_t *row_ptr, const int32_t *col, int64_t n_rows,
                                    int64_t nnz, uint64_t seed, const uint8_t *protect,
                                    int64_t *counts, int32_t *status, void *workspace,
                                    size_t workspace_bytes, void *stream);
int dw_edge_holdout_protected(const int64_t *row_ptr, const int32_t *col, const double *weights,
                              int64_t n_rows, int64_t nnz, uint64_t seed, const uint8_t *protect,
                              int64_t n_candidates, int64_t n_hold, int64_t *row_ptr_out,
                              int32_t *col_out, double *weights_out, int64_t *held,
                              int32_t *status, void *workspace, size_t workspace_bytes,
                              void *stream);

/* One pass of a multinomial logistic regression over the rows table[ids[i]], no float64 copy of
 * the features stored — what sklearn's LogisticRegression.fit / .predict compute from
 * X = embeddings[1:] in tools/graph_model_downstream_classification.py:58-86. coef
 * double[n_classes, dim + 1] (per class the weights, then the intercept; DEVICE memory), ids
 * int64[n], labels int32[n]. Per sample, with x the fp32 row widened exactly to float64:
 * z_k = w_k . x + b_k, m = max_k z_k, loss = m + log sum_k exp(z_k - m) - z_y,
 * r_k = softmax(z)_k - [k = y]. out double[n_classes * (dim + 1) + 2]:
 * [k * (dim + 1) + j] = sum r_k x_j for j < dim and sum r_k at j = dim, then sum loss, then the
 * number of samples whose argmax equals y. pred int32[n] (or NULL) receives the argmax, ties to
 * the lowest class. 1 <= dim <= 512, 2 <= n_classes <= 64, vocab_size < 2^31. Both products run
 * on v_mfma_f64_16x16x4_f64 over tiles of 16 samples; the class columns that pad n_classes to a
 * multiple of 16 take no part in the max or the sum, and a dim that is no multiple of 4, a table
 * that is not 16-B aligned and a short last tile take zero-filled operands. All sums float64 and
 * reproducible bit for bit: per-block partial rows in the workspace
 * (>= dw_node_softmax_workspace_bytes(n, dim, n_classes)) added in block order by a second
 * kernel, a grid that depends on (n, dim) only, no float atomics. An id outside [0, vocab_size)
 * or a label outside [0, n_classes) sets DW_S_BAD_INDEX: that sample contributes nothing to any
 * sum and its pred is -1 (nothing out of range is read). n = 0 writes nothing. */
int dw_node_softmax_workspace_bytes(int64_t n, int32_t dim, int32_t n_classes, size_t *bytes);
int dw_node_softmax(const float *table, int64_t vocab_size, int32_t dim, const int64_t *ids,
                    const int32_t *labels, int64_t n, int32_t n_classes, const double *coef,
                    double *out, int32_t *pred, void *workspace, size_t workspace_bytes,
                    int32_t *status, void *stream);

/* One pass of a one-vs-rest logistic regression over the rows table[ids[i]]: the multi-label
 * sibling of dw_node_softmax (a departure: the reference has no multi-label task), same staging,
 * same two float64 MFMA products, same accumulation order. masks uint64[n]: bit c of masks[i]
 * says sample i has label c; mask 0 is a valid sample of no label. 1 <= n_classes <= 64. A
 * sample whose id is outside [0, vocab_size) or whose mask has a bit at or above n_classes sets
 * DW_S_BAD_INDEX, contributes nothing to any sum and gets pred 0. Per sample and class c, with
 * y_c the mask's bit: z_c = w_c . x + b_c, loss = max(z_c, 0) - y_c z_c + log1p(exp(-|z_c|)),
 * r_c = sigmoid(z_c) - y_c, the sigmoid from exp(-|z_c|) (finite for every z). Predicted labels:
 * rule DW_OVR_THRESHOLD, every c with z_c > 0; rule DW_OVR_TOP_K, with k = popcount(masks[i]),
 * every c whose rank #{c' : z_c' > z_c, or z_c' = z_c and c' < c} is below k (ties to the lowest
 * class, k = 0 predicts nothing). pred uint64[n] (or NULL; the sums do not depend on it) receives
 * them as a mask. out double[K (dim + 1) + 1 + 3 K], K = n_classes:
 * [c * (dim + 1) + j] = sum r_c x_j for j < dim and sum r_c at j = dim, then the summed loss,
 * then tp[K] (samples with label c that are predicted c), predicted[K] and true[K], exact
 * integers. Reproducible bit for bit as dw_node_softmax is, the counts by integer adds. */
#define DW_OVR_THRESHOLD 0
#define DW_OVR_TOP_K 1
int dw_node_ovr_workspace_bytes(int64_t n, int32_t dim, int32_t n_classes, size_t *bytes);
int dw_node_ovr(const float *table, int64_t vocab_size, int32_t dim, const int64_t *ids,
                const uint64_t *masks, int64_t n, int32_t n_classes, const double *coef,
                int32_t rule, double *out, uint64_t *pred, void *workspace,
                size_t workspace_bytes, int32_t *status, void *stream);

/* One Lloyd pass of k-means over the rows table[ids[i]], no float64 copy of the features stored
 * (node2vec section 4.1 clusters the embeddings; a departure: the reference has no clustering
 * task). centroids double[n_clusters, dim] (DEVICE memory), ids int64[n]. Per sample, with x the
 * fp32 row widened exactly to float64: s_k = ||c_k||^2 - 2 x . c_k, label = argmin_k s_k (ties
 * to the lowest k), inertia term ||x||^2 + s_label. labels_out int32[n]; prev_labels int32[n] or
 * NULL. out double[K (dim + 1) + 2], K = n_clusters: [k * (dim + 1) + j] = the sum of x_j over
 * cluster k's members for j < dim and the member count at j = dim, then the summed inertia, then
 * the number of samples whose label differs from prev_labels[i] (n when prev_labels is NULL).
 * Counts are accumulated as integers and stored as doubles. 1 <= dim <= 512,
 * 1 <= n_clusters <= 1024, vocab_size < 2^31. An id outside [0, vocab_size) sets DW_S_BAD_INDEX:
 * its label is -1 and it contributes nothing to the sums, the counts or the inertia (it counts as
 * changed when -1 differs from its previous label); nothing out of range is read. n = 0 writes
 * nothing. Both products run on v_mfma_f64_16x16x4_f64 over tiles of 16 samples: the scores
 * X C^T against centroid tiles of 16 streamed with a running (min, argmin), padded centroid
 * columns taking no part, and the sums (one-hot)^T X per group of 64 clusters, each block's
 * accumulators in registers; a dim that is no multiple of 4, a table that is not 16-B aligned
 * and a short last tile take zero-filled operands as in dw_node_softmax. All sums float64 and
 * reproducible bit for bit: per-block partial rows in the workspace
 * (>= dw_kmeans_step_workspace_bytes(n, dim, n_clusters), 256-byte aligned) added in block order
 * by a last kernel, grids that depend on (n, dim, n_clusters) only, no float atomics. */
int dw_kmeans_step_workspace_bytes(int64_t n, int32_t dim, int32_t n_clusters, size_t *bytes);
int dw_kmeans_step(const float *table, int64_t vocab_size, int32_t dim, const int64_t *ids,
                   int64_t n, const double *centroids, int32_t n_clusters,
                   const int32_t *prev_labels, int32_t *labels_out, double *out, void *workspace,
                   size_t workspace_bytes, int32_t *status, void *stream);

/* k-means++ seeding (Arthur & Vassilvitskii 2007; the plain law, not sklearn's greedy variant)
 * over the rows table[ids[i]], n >= n_clusters. U_j = the Philox4x32-10 block of counter
 * (j, 0, 0, 0x4B4D0000) under key (seed lo, seed hi), words x, y joined as
 * ((x >> 5) << 26 | y >> 6) 2^-53. Centre 0 is sample floor(U_0 n). For centre j >= 1, D2[i] is
 * the squared distance (float64, columns in ascending order) from sample i to the nearest of
 * centres 0 .. j - 1, updated by one pass per centre, and the draw is the first sample with
 * D2 > 0 whose running sum of D2 exceeds U_j T (T the total; the sums are hierarchical: index
 * order inside a block of 256 samples, block order inside 256 chunks, chunk order), so sample i
 * is drawn with probability D2[i] / T. If every remaining D2 is zero — fewer distinct rows than
 * n_clusters — centre j is the lowest sample index not chosen yet. chosen_out int64[n_clusters]
 * receives the sample indices (into ids), centroids_out double[n_clusters, dim] their rows
 * widened. An id outside [0, vocab_size) sets DW_S_BAD_INDEX, has D2 = 0 and, if chosen, gives a
 * row of zeros. Workspace >= dw_kmeans_seed_workspace_bytes(n), 256-byte aligned. Reproducible
 * bit for bit; n = 0 writes nothing. */
int dw_kmeans_seed_workspace_bytes(int64_t n, size_t *bytes);
int dw_kmeans_seed(const float *table, int64_t vocab_size, int32_t dim, const int64_t *ids,
                   int64_t n, int32_t n_clusters, uint64_t seed, int64_t *chosen_out,
                   double *centroids_out, void *workspace, size_t workspace_bytes,
                   int32_t *status, void *stream);

/* The contingency table of two partitions: table_out int64[Ka, Kb] (zeroed here), cell [a, b] the
 * number of i with labels_a[i] = a and labels_b[i] = b, by integer atomics. Labels int32; -1 in
 * either array skips the sample; any other label outside its range sets DW_S_BAD_INDEX and
 * skips it. Ka Kb <= 2^24. n = 0 writes nothing. */
int dw_partition_counts(const int32_t *labels_a, int32_t n_a_classes, const int32_t *labels_b,
                        int32_t n_b_classes, int64_t n, int64_t *table_out, int32_t *status,
                        void *stream);

/* The integers of the structural (unweighted) modularity of labels int32[n_rows] over a CSR
 * graph, counted as networkx.community.modularity(G, parts, weight=None) does for the undirected
 * graph the symmetric CSR stores: out int64[2 K] (zeroed here), [2 c] the number of CSR entries
 * (u, v) with labels[u] = labels[v] = c and [2 c + 1] the summed degree of cluster c, a
 * self-loop entry (stored once) counting twice in both. Q = sum_c in_c / 2m - (deg_c / 2m)^2
 * with 2m = sum_c deg_c. A row of label -1 is skipped (its entries count for no cluster); a label
 * outside [-1, K), a column outside [0, n_rows) or a malformed row_ptr sets DW_S_BAD_INDEX and
 * skips the row. Weights are not read. n_rows = 0 writes nothing. */
int dw_modularity_counts(const int64_t *row_ptr, const int32_t *col, int64_t n_rows, int64_t nnz,
                         const int32_t *labels, int32_t n_clusters, int64_t *out, int32_t *status,
                         void *stream);

/* nn.Embedding(max_norm=...) lookup side effect (model.py:24-25 with max_norm set; torch
 * embedding_renorm_): every DISTINCT row among ids[0..n_ids) whose L2 norm exceeds max_norm is
 * scaled by max_norm / (norm + 1e-7), in place. Ids are deduplicated on the device (radix sort
 * in the caller's workspace, >= dw_embedding_renorm_workspace_bytes). Out-of-range ids set
 * DW_S_BAD_INDEX and are skipped. */
int dw_embedding_renorm_workspace_bytes(int64_t n_ids, int64_t vocab_size, size_t *bytes);
int dw_embedding_renorm(float *weight, int64_t vocab_size, int32_t dim, const int64_t *ids,
                        int64_t n_ids, double max_norm, void *workspace, size_t workspace_bytes,
                        int32_t *status, void *stream);

/* Bytes of device workspace the records path needs for n_centres centres with n_ctx contexts
 * and neg_samples negatives each over a vocabulary of vocab_size rows. */
int dw_sgns_workspace_bytes(int64_t n_centres, int32_t n_ctx, int32_t neg_samples,
                            int64_t vocab_size, size_t *bytes);

/* Walk aggregation (the walks forms on the records path: dw_sgns_walks, dw_sgns_walks_phase,
 * dw_sgns_walks_phase2_adam, dw_sgns_walks_phase2_piece). Position j of walk w is the context of
 * at most 2R centres, all of walk w, so its positive out-gradient terms are summed once per
 * (walk, position) — G[w][j] = sum_i coef(i, j) w_in[walk[w][i]], ascending i, fmaf, no atomics
 * (k_walk_agg, at the end of phase 1) — and enter the sort and the gather as ONE record in place
 * of up to 2R. Workspace layout when active: the negatives' records dense at
 * [0, n_centres * 2R * K), then one aggregate record per position at [.., + n_walks * L):
 * key walk[w][j], coefficient 1, centre field 1u << 31 | (w * L + j) (an id outside [0, V): key 0,
 * coefficient 0, DW_S_BAD_INDEX); then the positive coefficients (float[n_centres * 2R]) and
 * the aggregate rows (float[n_walks * L, dim]). g_in, the loss sums and the Philox keys are
 * those of the per-term records; g_out is the same sums reassociated.
 * Active when: dim in {64, 128, 256, 512} and 2R(1+K) <= 64 (the 16-lane-group pass 1),
 * n_walks * L < 2^31, k_walk_agg's staging ((L-2R) * min(dim,128) * 4 + (L-2R) * 2R * 4 + 4L B)
 * fits 64 KB of LDS, no deterministic accumulator (dw_exact_register) on g_out or g_in — that
 * mode keeps the per-term records; register both buffers or neither — and, in the auto mode,
 * 2R(L-2R) >= 2L (it at least halves the positive records).
 *
 * dw_sgns_walks_workspace_bytes: what the walks forms need for this shape with aggregation on or
 * off (>= dw_sgns_workspace_bytes of the same batch). A walks call whose workspace is too small
 * for its layout returns DW_E_INVALID_ARG.
 * dw_sgns_set_walk_agg: -1 auto (default; the initial mode is DW_SGNS_WALK_AGG = 0 / 1 from the
 * environment when set), 0 off, 1 on wherever supported (only the 2R(L-2R) >= 2L test is
 * skipped). Host state read at each call: the calls of one step must see one mode.
 * dw_sgns_walk_agg_active: 1 when a call of this shape aggregates under the current mode (no
 * deterministic accumulator assumed), else 0; bad sizes DW_E_INVALID_ARG. */
int dw_sgns_walks_workspace_bytes(int64_t n_walks, int32_t walk_length, int32_t context_radius,
                                  int32_t neg_samples, int64_t vocab_size, int32_t dim,
                                  size_t *bytes);
int dw_sgns_set_walk_agg(int32_t mode);
int dw_sgns_walk_agg_active(int64_t n_walks, int32_t walk_length, int32_t context_radius,
                            int32_t neg_samples, int32_t dim);

/* Profiling aid (bench.py): enable != 0 starts (and resets) per-phase HIP-event timing of every
 * later dw_sgns_walks / dw_sgns_pairs call on this process; enable == 0 stops it.
 * dw_sgns_phase_ms waits for the last recorded call and returns the mean milliseconds of
 * ms[0] pass 1 (k_sgns*: logits, loss, centre gradients, records), ms[1] the radix sort of the
 * records, ms[2] pass 2 (k_rec_gather: output-table gradients) over *n_calls calls (ms[1],
 * ms[2] are 0 in atomic mode). No reference counterpart (measurement only). */
int dw_sgns_timing(int32_t enable);
int dw_sgns_phase_ms(double *ms, int64_t *n_calls);

/* CBOW.forward(inputs, outputs, proba) (model.py:98-110): logits[b, n] =
 * <mean_p w_in[inputs[b, p]], w_out[outputs[b, n]]>, p < n_in; dw_skipgram_logits is n_in = 1.
 * The backward adds dlogits[b,n] * pooled_b into g_out[outputs[b,n]] and (sum_n dlogits[b,n] *
 * w_out[outputs[b,n]]) / n_in into each g_in[inputs[b, p]]. */
int dw_pooled_logits(const int64_t *inputs, int32_t n_in, const int64_t *outputs,
                     int64_t batch, int32_t n_out, int64_t vocab_size, int32_t dim,
                     const float *w_in, const float *w_out, int32_t proba, float *logits,
                     int32_t *status, void *stream);
int dw_pooled_logits_backward(const int64_t *inputs, int32_t n_in, const int64_t *outputs,
                              int64_t batch, int32_t n_out, int64_t vocab_size, int32_t dim,
                              const float *w_in, const float *w_out, const float *dlogits,
                              float *g_in, float *g_out, int32_t *status, void *stream);

/* SkipGram.forward(inputs, outputs, proba) (model.py:79-91): logits[b, n] =
 * <w_in[inputs[b]], w_out[outputs[b, n]]>, sigmoid applied when proba != 0. */
int dw_skipgram_logits(const int64_t *inputs, const int64_t *outputs, int64_t batch,
                       int32_t n_out, int64_t vocab_size, int32_t dim, const float *w_in,
                       const float *w_out, int32_t proba, float *logits, int32_t *status,
                       void *stream);

/* Backward of dw_skipgram_logits (proba == 0): g_in[inputs[b]] += sum_n dlogits[b,n] w_out[..],
 * g_out[outputs[b,n]] += dlogits[b,n] w_in[inputs[b]] (the embedding_dense_backward of
 * model.py:85-88 under autograd). */
int dw_skipgram_logits_backward(const int64_t *inputs, const int64_t *outputs, int64_t batch,
                                int32_t n_out, int64_t vocab_size, int32_t dim,
                                const float *w_in, const float *w_out, const float *dlogits,
                                float *g_in, float *g_out, int32_t *status, void *stream);

/* Dense Adam step, torch.optim.Adam single-tensor semantics (torch/optim/adam.py:_single_tensor_adam,
 * amsgrad=False), configured by config_parser/core.py:43-53. Host computes the per-step scalars
 * in float64 exactly as torch does; the kernel runs the fp32 tensor ops:
 *   m = lerp(m, g, one_minus_beta1); v = v*beta2 + one_minus_beta2*g*g;
 *   denom = sqrt(v)/bias_correction2_sqrt + eps; p += neg_step_size * m/denom;
 * weight_decay != 0 adds weight_decay*p to g first (L2, non-decoupled).
 * zero_grad != 0 also writes g = 0 (fuses optimizer.zero_grad into the same HBM pass). */
int dw_adam_dense(float *param, float *grad, float *exp_avg, float *exp_avg_sq, int64_t n_elem,
                  float one_minus_beta1, float beta2, float one_minus_beta2,
                  float bias_correction2_sqrt, float neg_step_size, float eps,
                  float weight_decay, int32_t zero_grad, void *stream);

/* dw_adam_dense reading the parameters from param_src and writing them to param_dst (the other
 * buffer of a double-buffered table, so readers of the current values can run concurrently);
 * param_src == param_dst is dw_adam_dense. max_blocks > 0 caps the grid (256-thread blocks,
 * grid-stride): a concurrent kernel on another stream keeps the rest of the CUs; <= 0 = the
 * full grid. */
int dw_adam_dense_to(const float *param_src, float *param_dst, float *grad, float *exp_avg,
                     float *exp_avg_sq, int64_t n_elem, float one_minus_beta1, float beta2,
                     float one_minus_beta2, float bias_correction2_sqrt, float neg_step_size,
                     float eps, float weight_decay, int32_t zero_grad, int64_t max_blocks,
                     void *stream);

/* Dense SGD step, torch.optim.SGD single-tensor semantics (torch/optim/sgd.py:_single_tensor_sgd,
 * maximize=False), for configs whose `train.optimizer._target_` names it (the reference's
 * config_parser/core.py:43-53 instantiates whatever optimizer the config names). The host
 * prepares the scalars in float64 and casts them to float32: neg_lr = -lr, weight_decay,
 * momentum, one_minus_dampening = 1 - dampening. Per element, every fma a single rounding:
 *   g1  = weight_decay != 0 ? fma(weight_decay, p, g) : g
 *   buf = first_step ? g1 : fma(one_minus_dampening, g1, RN(momentum * buf))   (momentum != 0)
 *   g2  = momentum == 0 ? g1 : nesterov ? fma(momentum, buf, g1) : buf
 *   p   = fma(neg_lr, g2, p)
 * which is torch's update on CPU fp32 tensors bit for bit (tests/test_sgd.py).
 * momentum_buf: NULL iff momentum == 0 (torch's state `momentum_buffer`; first_step != 0 writes
 * it without reading it). zero_grad != 0 also writes g = 0 in the same pass. One streaming pass,
 * 16-B accesses where the buffers are 16-B aligned, any n_elem >= 0. */
int dw_sgd_dense(float *param, float *grad, float *momentum_buf, int64_t n_elem, float neg_lr,
                 float weight_decay, float momentum, float one_minus_dampening, int32_t nesterov,
                 int32_t first_step, int32_t zero_grad, void *stream);

/* Plain SGD (momentum = weight_decay = 0) over the rows a batch touched: for every distinct row r
 * in ids, p[r] = fma(neg_lr, g[r], p[r]) and g[r] = 0 (the arithmetic of dw_sgd_dense, the same
 * bits). A row with g = 0 does not move under plain SGD, so with ids a superset of the rows that
 * hold a gradient this is the whole step, with nothing dense in it.
 *   param, grad: float32 [n_table_rows, dim], dim >= 1 (rows are stepped with the widest of
 *         16-, 8- and 4-B accesses that dim and the buffers' alignment keep aligned for every row);
 *   ids:  n_ids row ids, int32 (id_bytes 4) or int64 (id_bytes 8), in any order, duplicates in
 *         any number: each distinct row is stepped once. An id outside [0, n_table_rows) is
 *         skipped and sets DW_S_BAD_INDEX in status;
 *   claim: uint32 [ceil(n_table_rows / 32)], all zero on entry and left all zero (cleared on the
 *         stream behind the step): one bit per row, taken by the first lister of the row;
 *   neg_lr = -lr <= 0.
 * A row not listed keeps its p and g bit for bit; so does a listed row whose gradient is all +0
 * (nothing is written for it). Two launches (the step, the bitmap clear) whose geometry depends
 * only on (n_ids, n_table_rows, dim); no synchronisation, no allocation, no host read: the call
 * can be captured in a HIP graph. n_ids == 0 is a no-op. */
int dw_sgd_rows(float *param, float *grad, int64_t n_table_rows, int32_t dim, const void *ids,
                int32_t id_bytes, int64_t n_ids, uint32_t *claim, float neg_lr, int32_t *status,
                void *stream);

/* Scale a float32 buffer in place: x *= alpha * (*alpha_dev) (alpha_dev NULL -> 1). Used by the
 * autograd path to apply the device-resident grad_output without a host synchronisation. */
/* Lazy exact Adam over selected rows (OwnerLazyTables, the touched-row in-table exchange;
 * torch.optim.Adam single-tensor semantics as dw_adam_dense). A row's update with g = 0 is a
 * fixed recurrence, so rows no batch touched are brought up to date later by replaying each
 * missed step through the same per-element arithmetic: the result is bit-identical to the
 * dense update every step.
 *   rows: uint32 row ids (NULL = rows 0 .. n_rows_max-1); n_rows_dev: device int64 count
 *         (NULL = n_rows_max; clamped to n_rows_max); ids >= n_table_rows are skipped;
 *   last_step: int32[n_table_rows], the step each row's (param, exp_avg, exp_avg_sq) are
 *         current to; updated;
 *   hist: float32[(step+1) * 8]: row s = Adam step s's scalars in dw_adam_dense's order
 *         (1-beta1, beta2, 1-beta2, sqrt(bias_correction2), -lr/bias_correction1, eps,
 *         weight_decay), then fp32 1 / sqrt(bias_correction2) correctly rounded (0 = not given:
 *         the kernels divide; given, they take three operations for the same quotient);
 *         row 0 (no step) may hold the box header: [0] = the bits of DW_HIST_BOX_TAG, [1] = the
 *         bits of an int32 step b such that every row s >= b up to the last one a launch reads
 *         has weight_decay +0, the reciprocal, eps in [2^-27, 1], sqrt(bias_correction2) in
 *         [2^-10, 1] and 1-beta1, beta2 in [0, 1]: the g = 0 replays of rows last current at
 *         b - 1 or later then run sqrt and the division without range scaling (the same bits,
 *         fewer operations); [2] = F, [3] = eps of those rows: with every box row's eps equal to
 *         it, (1 - beta1)(1 + 2^-20) <= sqrt(beta2) and |nstep| <= F, a replay whose parameter
 *         can provably no longer move (|m| F / max(RN(sqrt(v)), eps) below |p| 2^-26) steps m
 *         and v alone for the rest of the run (the same bits; F = +inf, or any F that is not a
 *         positive number — 0, negative, NaN, so also zeros left behind [0] and [1]: never; under
 *         the latter [3]..[5] are not read at all); [4] = 1-beta1,
 *         [5] = beta2 when every box row has those same values (the frozen steps then take them
 *         from here, not from each row; NaN = the betas vary); any other row 0 = no step in the
 *         box;
 *   grad_rows NULL: replay every listed row up to `step` (g = 0);
 *   grad_rows float32[n_rows_max, dim]: replay up to step - 1, then apply `step` with row i's
 *         gradient grad_rows[i];
 *   grad_by_row (with grad_rows): grad_rows is the table's dense gradient [n_table_rows, dim]
 *         and row r steps with grad_rows[r], which is cleared as it is read (one rank's touched
 *         rows: no gather);
 *   pending: NULL, or uint8 [n_table_rows] (dw_sgns_owner_out_rows): a listed row marked there
 *         first gets the parameter half of step last_step[r], and its mark is cleared; only
 *         with grad_rows NULL (a settle-and-replay: a gradient step on a pending row current to
 *         `step` would apply that step twice) — DW_E_INVALID_ARG otherwise. */
int dw_adam_rows(float *param, float *exp_avg, float *exp_avg_sq, int32_t *last_step,
                 uint8_t *pending, int64_t n_table_rows, int32_t dim, const uint32_t *rows,
                 const int64_t *n_rows_dev, int64_t n_rows_max, float *grad_rows,
                 int32_t grad_by_row, const float *hist, int32_t step, void *stream);

/* out[i] = table[rows[i]] for i < min(*n_rows_dev, n_rows_max) (float32 rows of dim); with
 * zero_source the table rows are cleared in the same pass (the touched rows of the in-table
 * gradient, gathered for the all-reduce). */
int dw_rows_gather(float *table, int64_t n_table_rows, int32_t dim, const uint32_t *rows,
                   const int64_t *n_rows_dev, int64_t n_rows_max, float *out,
                   int32_t zero_source, void *stream);

int dw_scale(float *x, int64_t n_elem, float alpha, const float *alpha_dev, void *stream);

/* ---- step scalars in device memory (HIP-graph replay of a training step) ------------------------
 * A small-batch training step is a few dozen microseconds of kernels; launched one by one from
 * the host it is launch-bound. To replay a captured step (hipGraph), the values that change from
 * step to step live in device memory instead of kernel arguments: while a dw_step_scalars block
 * is BOUND (dw_step_scalars_bind, per host thread), every launch of
 *   dw_walk_fast / dw_walk_fast_indexed / dw_walk_fast_positions   reads walk_id0 from it,
 *   dw_sgns_walks_phase (pass 1), dw_sgns_noise_alias   read noise_offset from it,
 *   dw_adam_dense(_to), dw_sgns_walks_phase2_adam   read the Adam scalars adam[0..6],
 * and ignores the corresponding host arguments. dw_step_scalars_advance, the last node of a
 * captured step, moves the block to the next step. Nothing else changes: the kernels and their
 * results are those of the eager launches (the bench and tests compare the two). Replaces no
 * reference interface: it is how trainer.py:131-152's per-batch step is replayed on the device. */
typedef struct dw_step_scalars {
    uint64_t walk_id0;      /* global walk id of the step's first walk */
    uint64_t noise_offset;  /* centre counter of the step's device negatives */
    int64_t step;           /* the Adam step this step applies (1-based) */
    float adam[8];          /* its scalars, dw_adam_dense order, then RN(1/bias_correction2_sqrt) or 0 (a dw_adam_rows hist row) */
} dw_step_scalars;

/* Bind (dev != NULL) or unbind (NULL) a device dw_step_scalars for the launches this host
 * thread makes next. */
int dw_step_scalars_bind(const dw_step_scalars *dev);

/* As dw_step_scalars_bind, and the launches' Adam step numbers become relative to the block:
 * dw_adam_rows, dw_sgns_owner_out_catch_up and dw_sgns_owner_pass2_lazy then apply
 * dev->step + (step - host_step), read on the device, where `step` is their argument (the lazy
 * exact Adam of a captured one-GPU owner step: word2vec/graphed.py GraphedOwnerStep). Those
 * three refuse (DW_E_INVALID_ARG) a block bound without its host step. */
int dw_step_scalars_bind_at(const dw_step_scalars *dev, int64_t host_step);

/* walk_id0 += walks_per_step, noise_offset += centres_per_step, step += 1, adam = hist[step]
 * (hist: float32[hist_rows][8]; a step beyond hist_rows sets DW_S_BAD_INDEX in status and
 * leaves adam unchanged); then, with epoch_starts != NULL, the new step's start nodes into
 * starts_out exactly as dw_step_starts (one launch for both). */
int dw_step_scalars_advance(dw_step_scalars *dev, const float *hist, int64_t hist_rows,
                            uint64_t walks_per_step, uint64_t centres_per_step, int32_t *status,
                            const int32_t *epoch_starts, int64_t n_epoch, int32_t *starts_out,
                            int64_t n, void *stream);

/* Several steps in one launch (a graph that replays n_steps steps): steps[j] = *base advanced j
 * times as dw_step_scalars_advance would (j = 0 .. n_steps-1), then *base advanced n_steps
 * times; with epoch_starts != NULL, starts_out[k] = epoch_starts[(steps[0].walk_id0 + k) mod
 * n_epoch] for k < n (the start nodes of all n_steps steps' walks). Binding &steps[j] for step
 * j's launches replaces the n_steps advance launches of a captured multi-step graph. */
int dw_step_scalars_expand(dw_step_scalars *base, dw_step_scalars *steps, int64_t n_steps,
                           const float *hist, int64_t hist_rows, uint64_t walks_per_step,
                           uint64_t centres_per_step, int32_t *status,
                           const int32_t *epoch_starts, int64_t n_epoch, int32_t *starts_out,
                           int64_t n, void *stream);

/* starts_out[k] = epoch_starts[(dev->walk_id0 + k) mod n_epoch] for k < n: the start nodes of
 * a step's walks when walk w of the epoch starts at epoch_starts[w] (RandomWalkDataset's
 * `_get_current_node`, datasets.py:69-76, with the walk ids of the epoch). */
int dw_step_starts(const dw_step_scalars *dev, const int32_t *epoch_starts, int64_t n_epoch,
                   int32_t *starts_out, int64_t n, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* DW_HIP_H */
