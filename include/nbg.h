/*
 * nbg.h — C ABI of nebula_amd, the MI355X-native multi-hop traversal engine for Nebula Graph's
 * GO N STEPS / FIND PATH hot path.
 *
 * Plain C, no exceptions, no callbacks, no torch types.  Every entry point returns an int32_t
 * status: 0 on success, otherwise a storage::cpp2::ErrorCode / graph::cpp2::ErrorCode value
 * (src/interface/storage.thrift:13-44, graph.thrift:12-35) or one of the NBG_E_* codes below.
 * The caller owns every input; outputs are allocated by the library and released with the
 * matching *_free call.  Engines are immutable after nbg_finalize(); queries on one engine are
 * serialised internally (one HIP stream per engine).
 *
 * Reference interfaces this ABI replaces (paths relative to the reference checkout):
 *   nbg_create/…/nbg_finalize  ≙ the storaged data a kvstore part holds: NebulaStore parts
 *       filled through AddEdgesProcessor / AddVerticesProcessor
 *       (src/storage/AddEdgesProcessor.cpp:15-37, src/kvstore/NebulaStore.cpp:326-336)
 *   nbg_go / nbg_go_device     ≙ GoExecutor result semantics (src/graph/GoExecutor.cpp:83-984)
 *   nbg_go_prepare / _execute  ≙ GoExecutor::prepare() / execute() (GoExecutor.cpp:28-110)
 *   nbg_go_piped               ≙ GoExecutor::setupStarts over piped rows (GoExecutor.cpp:365-399,
 *                                InterimResult::getVIDs / buildIndex, src/graph/InterimResult.cpp:29-250)
 *   nbg_find_path              ≙ FindPathExecutor result semantics
 *       (src/graph/FindPathExecutor.cpp:145-715)
 *   nbg_group_by               ≙ GroupByExecutor (src/graph/GroupByExecutor.cpp:181-322,
 *       AggregateFunction.h)
 *   nbg_order_by               ≙ OrderByExecutor + LimitExecutor (src/graph/OrderByExecutor.cpp:14-155,
 *       src/graph/LimitExecutor.cpp:18-66)
 *   nbg_set_op                 ≙ SetExecutor (src/graph/SetExecutor.cpp:98-383)
 *   nbg_yield                  ≙ YieldExecutor over piped rows (src/graph/YieldExecutor.cpp:178-282)
 *   nbg_yield_agg              ≙ YieldExecutor with aggregate functions and no GROUP BY
 *       (src/graph/YieldExecutor.cpp:33-58, 178-282, AggregateFunction.h)
 *   nbg_fetch_vertices         ≙ FetchVerticesExecutor over piped rows or a vid list
 *       (src/graph/FetchVerticesExecutor.cpp:19-311, src/graph/FetchExecutor.cpp:14-131)
 *   nbg_fetch_edges ≙ FetchEdgesExecutor (src/graph/FetchEdgesExecutor.cpp:17-384, src/graph/FetchExecutor.cpp:14-131, src/storage/QueryEdgePropsProcessor.cpp:17-101)
 *   nbg_rows_encode ≙ GoExecutor::setupInterimResult / RowSetWriter (src/graph/GoExecutor.cpp:707-779)
 *   nbg_rows_decode ≙ InterimResult::getRows / RowSetReader + RowReader
 *       (src/graph/InterimResult.cpp:74-250, src/dataman/RowReader.cpp:213-258, RowSetReader.cpp)
 *   nbg_get_neighbors          ≙ StorageServiceHandler::future_getBound → QueryBoundProcessor
 *       (src/storage/StorageServiceHandler.cpp:33-40, src/storage/QueryBoundProcessor.cpp:16-220)
 */
#ifndef NEBULA_AMD_NBG_H_
#define NEBULA_AMD_NBG_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (storage.thrift ErrorCode / graph.thrift ErrorCode values) ---------- */
#define NBG_OK                     0
#define NBG_E_SYNTAX_ERROR        (-7)    /* graph.thrift E_SYNTAX_ERROR */
#define NBG_E_EXECUTION_ERROR     (-8)    /* graph E_EXECUTION_ERROR: eval error in WHERE/YIELD */
#define NBG_E_PART_NOT_FOUND      (-14)
#define NBG_E_EDGE_PROP_NOT_FOUND (-21)
#define NBG_E_TAG_PROP_NOT_FOUND  (-22)
#define NBG_E_IMPROPER_DATA_TYPE  (-23)
#define NBG_E_INVALID_FILTER      (-31)
#define NBG_E_UNKNOWN             (-100)
/* nebula_amd specific */
#define NBG_E_INVALID_ARGUMENT    (-1001)
#define NBG_E_UNSUPPORTED         (-1002) /* valid nGQL, not implemented on the device path */
#define NBG_E_DEVICE              (-1003) /* HIP runtime / kernel failure (message in last_error) */
#define NBG_E_OUT_OF_MEMORY       (-1004)
#define NBG_E_STATE               (-1005) /* e.g. query before nbg_finalize */

/* ---- Device limits ----------------------------------------------------------------------
 * A statement past one of these returns NBG_E_UNSUPPORTED before any row is produced (on every
 * rank of a partitioned engine), so the caller can run the reference's own executor on it
 * (tests/test_gpu_limits.py holds one test per limit):
 *   more than NBG_MAX_YIELDS YIELD columns; more than NBG_MAX_OVER OVER types (OVER * included;
 *   GO, FIND PATH, GetNeighbors); a WHERE + YIELD program over 256 instructions or 16 live
 *   registers per OVER type; GO over 32 STEPS; FIND SHORTEST PATH UPTO over 63, FIND ALL PATH
 *   UPTO over 32; $$ of a tag registered 17th or later; more than 32 $- / $var input columns.
 * nbg_group_by (tests/test_gpu_groupby.py holds one test per limit a GO result can reach; the last
 * two and the mixed-kind column are guards no GO result reaches today):
 *   a group or yield expression that is neither a bare `$-.col' nor constant-foldable;
 *   a referenced input column whose value kind differs between OVER types (col_kind == -1);
 *   an input whose row schema re-reads its columns (a misaligned or FLOAT column);
 *   AVG over a VID or TIMESTAMP column (the reference reads the wrong union member there);
 *   MAX / MIN over a string column that can hold strings outside the dictionary;
 *   more than NBG_MAX_YIELDS group columns or yield columns;
 *   a partitioned engine (num_gpus > 1): its rows live on several ranks;
 *   a carried-over string column whose OVER types spell different constants outside the dictionary;
 *   2^32 groups or more (group ids are 32 bits).
 * nbg_order_by (tests/test_gpu_orderby.py holds one test per limit a GO result can reach; the
 * mixed-kind column is a guard no GO result reaches today):
 *   a partitioned engine (num_gpus > 1): its rows live on several ranks;
 *   an input whose row schema re-reads its columns (a misaligned or FLOAT column);
 *   a column whose value kind differs between OVER types (col_kind == -1): a factor cannot be
 *   ordered, and the one-segment result gives every column one kind;
 *   a string factor column that can hold strings outside the dictionary (a non-empty derived
 *   table, or a per-OVER-type string constant for that column);
 *   a carried-over string column whose OVER types spell different constants outside the dictionary;
 *   more than NBG_MAX_YIELDS factors; a result of 2^32 rows or more.
 * nbg_set_op (tests/test_gpu_setops.py holds one test per limit a GO result can reach; the
 * mixed-kind column and the row counts are guards no test reaches):
 *   a partitioned engine (num_gpus > 1): its rows live on several ranks;
 *   an input whose row schema re-reads its columns (a misaligned or FLOAT column);
 *   a column whose value kind differs between OVER types (col_kind == -1);
 *   a string column carrying a per-OVER-type constant outside the dictionary, on either side (its
 *   code is private to its result, so the two inputs cannot be compared);
 *   a column pair where exactly one side is STRING (the cast formats or parses strings);
 *   a result of 2^32 rows or more; INTERSECT with a right input of 2^31 rows or more (a value's
 *   multiplicity is a signed 32-bit counter).
 *   The pass-through shortcuts have nbg_order_by's limits for the side passed on.
 * nbg_yield (tests/test_gpu_yield.py holds one test per limit a GO result can reach; the mixed-kind
 * column, the differently spelt constants and the row count are guards no test reaches):
 *   a partitioned engine (num_gpus > 1): its rows live on several ranks;
 *   any aggregate function (yield_funs[i] != NBG_AGG_NONE): whole-input aggregates without GROUP BY;
 *   (nbg_yield_agg below is the call for those requests;)
 *   a WHERE or YIELD that builds a string (concatenation, a cast to string, string functions);
 *   any use other than a bare pass-through column of a string column that can hold strings outside
 *   the dictionary (a non-empty derived table, or a per-OVER-type constant outside the dictionary);
 *   a passed-through string column whose OVER types spell different constants outside the dictionary;
 *   a referenced column whose value kind differs between OVER types (col_kind == -1);
 *   an input whose row schema re-reads its columns (a misaligned or FLOAT column);
 *   more than NBG_MAX_YIELDS columns after `$-.*' expansion; a program over 256 instructions or
 *   over the interpreter's register limit; an input of 2^32 rows or more.
 * nbg_yield_agg (tests/test_gpu_yield_agg.py holds one test per limit a GO result can reach; the
 * mixed-kind column, the string expression that builds no string and the row count are guards no
 * test reaches):
 *   a partitioned engine (num_gpus > 1): its rows live on several ranks;
 *   a column without a function that is not constant-foldable (`$-.w + 1' without a function, for
 *   which the reference reports the last kept row's value; rand32(); now());
 *   AVG over a TIMESTAMP-typed argument (the reference reads the wrong union member there);
 *   an argument or WHERE that builds a string (concatenation, a cast to string, string functions);
 *   MAX / MIN / COUNT_DISTINCT over a string argument that is anything but a constant or a bare
 *   column, or over a bare string column that can hold strings outside the dictionary; any use
 *   inside an expression of such a column;
 *   a referenced column whose value kind differs between OVER types (col_kind == -1);
 *   an input whose row schema re-reads its columns (a misaligned or FLOAT column);
 *   more than NBG_MAX_YIELDS columns after `$-.*' expansion; a program over 256 instructions, or
 *   whose registers and accumulator slots together are over the interpreter's register limit (a
 *   slot per distinct (argument, fold): one for SUM / AVG, MAX, MIN and each BIT_*, two for STD);
 *   an input of 2^32 rows or more.
 * nbg_fetch_vertices (tests/test_gpu_fetch.py holds one test per limit a GO result can reach; the
 * mixed-kind vid column, the missing tag tables and the row count are guards no test reaches):
 *   a partitioned engine (num_gpus > 1): its rows live on several ranks;
 *   an input whose row schema re-reads its columns (a misaligned or FLOAT column);
 *   a vid column whose value kind differs between OVER types (col_kind == -1);
 *   a YIELD that builds a string (concatenation, a cast to string, string functions);
 *   any prop for which nbg_go's compiler answers `$^.tag.prop' with NBG_E_UNSUPPORTED (a tag
 *   without device tables); a bare FLOAT prop (the result would carry a FLOAT column; below the
 *   root of an expression a FLOAT prop is accepted and reads as its double, a DOUBLE column);
 *   more than NBG_MAX_YIELDS columns; a program over 256 instructions or over the interpreter's
 *   register limit; an input of 2^32 rows or more.
 * nbg_fetch_edges (tests/test_gpu_fetch_edges.py holds one test per limit a GO result can reach; the
 * mixed-kind key column, the missing CSR and the row count are guards no test reaches):
 *   a partitioned engine (num_gpus > 1): its rows live on several ranks;
 *   an input whose row schema re-reads its columns (a misaligned or FLOAT column);
 *   a key column (src, dst or rank) whose value kind differs between OVER types (col_kind == -1);
 *   a YIELD that builds a string (concatenation, a cast to string, string functions);
 *   a bare FLOAT prop (the result would carry a FLOAT column; below the root of an expression a
 *   FLOAT prop is accepted and reads as its double, a DOUBLE column);
 *   more than NBG_MAX_YIELDS columns; a program over 256 instructions or over the interpreter's
 *   register limit; an input of 2^32 rows or more; an edge type without a device CSR (registered,
 *   but no edge of it was loaded).
 * nbg_go_piped (tests/test_gpu_go_piped.py holds one test per limit a GO result can reach; the
 * mixed-kind columns and the row count are guards no test reaches):
 *   a partitioned engine (num_gpus > 1): its rows live on several ranks;
 *   an input whose row schema re-reads its columns (a misaligned or FLOAT column);
 *   a FROM column, or a column referenced by WHERE / YIELD, whose value kind differs between OVER
 *   types (col_kind == -1);
 *   a referenced string column that can hold strings outside the dictionary (a non-empty derived
 *   table, or a per-OVER-type constant outside the dictionary): the host route gives such strings a
 *   table of their own, which the device index does not build;
 *   an input of 2^32 rows or more.
 *   nbg_go's own limits stay, among them the 2^32 - 1 bound on the start list's entries plus edges,
 *   which a piped list with duplicated hubs reaches easily (YIELD DISTINCT de-duplicates the list).
 * nbg_rows_encode (tests/test_gpu_rows_encode.py holds one test per limit a GO result can reach; the
 * mixed-kind column, the kind its type does not read, the row count and the 4 GiB row are guards no
 * test reaches):
 *   a partitioned engine (num_gpus > 1): its rows live on several ranks;
 *   an input whose row schema re-reads its columns (a misaligned or FLOAT column);
 *   a column whose value kind differs between OVER types (col_kind == -1), or is not the kind its
 *   type's reader takes (no aligned result has one);
 *   a string column that can hold strings outside the dictionary other than a per-OVER-type
 *   constant (a non-empty derived table);
 *   an input of 2^32 rows or more; a schema and dictionary under which one row could encode to
 *   4 GiB or more (a row's length is a 32-bit word between the passes).
 * nbg_rows_decode (tests/test_gpu_rows_decode.py holds one test per limit a test can reach; the row
 * count and the 4 GiB chunk are guards no test reaches):
 *   a partitioned engine (num_gpus > 1): its rows would live on several ranks;
 *   a FLOAT field: the aligned result has no FLOAT column (InterimResult::getRows fails on it too);
 *   more than NBG_MAX_YIELDS fields;
 *   an input of 2^32 rows or more; a chunk of 2,048 rows whose bytes reach 4 GiB (a row's start is
 *   a 32-bit offset from its chunk's);
 *   a STRING cell whose bytes are not in the snapshot's dictionary (the empty string is always
 *   there): the host route gives such strings a table of their own, which the device does not
 *   build yet.
 * (A storage filter with a function call is E_INVALID_FILTER per part, as checkExp answers it,
 * QueryBaseProcessor.inl:172-290.)
 * Not limits: $- / $var input strings absent from the snapshot's dictionary, string functions
 * nested to any depth in GO (both lifted in round 6). */
#define NBG_MAX_YIELDS 32
#define NBG_MAX_OVER   32

/* ---- common.thrift SupportedType ------------------------------------------------------ */
#define NBG_T_BOOL      1
#define NBG_T_INT       2
#define NBG_T_VID       3
#define NBG_T_FLOAT     4
#define NBG_T_DOUBLE    5
#define NBG_T_STRING    6
#define NBG_T_TIMESTAMP 7

/* Value tags of result cells: VariantType alternatives (src/common/base/Base.h:140). */
#define NBG_V_INT    0
#define NBG_V_DOUBLE 1
#define NBG_V_BOOL   2
#define NBG_V_STRING 3

typedef struct nbg_engine nbg_engine;
typedef struct nbg_rows nbg_rows;
typedef struct nbg_paths nbg_paths;

typedef struct {
  int32_t num_parts;     /* partition_num of the space: part = uint64(vid) % num_parts + 1   */
  int32_t num_gpus;      /* G: part p is served by GPU rank p % G (CreateSpaceProcessor:84-95) */
  int32_t rank;          /* this engine's GPU rank in [0, G)                                   */
  int32_t device;        /* HIP device ordinal to use                                          */
  int32_t max_edge_returned_per_vertex; /* FLAGS_max_edge_returned_per_vertex (INT32_MAX)       */
  int32_t min_vertices_per_bucket;      /* accepted for flag parity; no device effect           */
  int32_t max_handlers_per_req;         /* accepted for flag parity; no device effect           */
} nbg_config;

typedef struct {
  const char* name;
  int32_t type;          /* NBG_T_* */
} nbg_column_def;

/* ---- engine lifecycle ------------------------------------------------------------------ */
int32_t nbg_create(const nbg_config* cfg, nbg_engine** out);
void nbg_destroy(nbg_engine* e);
/* Message of the last failing call on this engine (valid until the next call). */
const char* nbg_last_error(const nbg_engine* e);

/* Schemas (meta SchemaManager view, src/meta/SchemaManager.h:20-48). */
int32_t nbg_register_tag(nbg_engine* e, int32_t tag_id, const char* name, int64_t schema_ver,
                         const nbg_column_def* cols, int32_t ncols);
int32_t nbg_register_edge(nbg_engine* e, int32_t edge_type, const char* name, int64_t schema_ver,
                          const nbg_column_def* cols, int32_t ncols);

/* Loader: KV records exactly as a kvstore part holds them — NebulaKeyUtils keys
 * (src/common/base/NebulaKeyUtils.cpp:12-47) and RowWriter values (src/dataman/RowWriter.cpp).
 * Record i is key_data[key_offs[i] .. key_offs[i+1]) / val_data[val_offs[i] .. val_offs[i+1]).
 * Later records with an identical key overwrite earlier ones (write-batch semantics).
 * Records of parts this rank does not serve (part % num_gpus != rank) are ignored. */
int32_t nbg_load_part_kv(nbg_engine* e, int32_t part,
                         const uint8_t* key_data, const uint64_t* key_offs,
                         const uint8_t* val_data, const uint64_t* val_offs, uint64_t n);

/* SST-file ingest: RocksDB BlockBasedTable files as rocksdb::SstFileWriter writes them for the
 * Spark generator (src/tools/spark-sstfile-generator/.../SstFileOutputFormat.scala:150-202),
 * replacing StorageHttpIngestHandler -> NebulaStore::ingest -> RocksEngine::ingest
 * (src/storage/StorageHttpIngestHandler.cpp:94-100, src/kvstore/NebulaStore.cpp:436-466,
 * src/kvstore/RocksEngine.cpp:360-370).  Every Put record is loaded as by nbg_load_part_kv (a key
 * already loaded is overwritten: the ingested file is newer).  Before nbg_finalize.
 *   nbg_ingest_sst: one file into `part`;
 *   nbg_ingest_dir: every "*.sst" under <download_dir>/<part>/ (recursively, in name order) for
 *                   every part this engine serves; a missing part directory is skipped.
 * Block compression none / Snappy; NBG_E_UNSUPPORTED for other codecs, record types other than
 * Put and format_version > 3; NBG_E_INVALID_ARGUMENT for unreadable or corrupt files (checksums
 * are verified). */
int32_t nbg_ingest_sst(nbg_engine* e, int32_t part, const char* path);
int32_t nbg_ingest_dir(nbg_engine* e, const char* download_dir);

/* Bulk loader (SST-ingest analogue): n edges of one positive edge type, inserted the way
 * InsertEdgeExecutor does (out-edge with props + in-edge (dst,-type,rank,src) with no props,
 * src/graph/InsertEdgeExecutor.cpp:180-196), all with one version; a later duplicate
 * (src,dst,rank) overwrites an earlier one.  prop_cols[c] points at n values of schema column c:
 * int64 for INT/TIMESTAMP/VID, double for FLOAT/DOUBLE, uint8 for BOOL; STRING columns are not
 * accepted here (use nbg_load_part_kv).  rank may be NULL (all 0). */
int32_t nbg_load_edges(nbg_engine* e, int32_t edge_type, const int64_t* src, const int64_t* dst,
                       const int64_t* rank, uint64_t n, const void* const* prop_cols, int32_t ncols);

/* Build the device snapshot (version de-dup, CSR/CSC per edge type, SoA prop columns) and upload
 * it to HBM.  Host-side staging is released afterwards. */
int32_t nbg_finalize(nbg_engine* e);

/* Snapshot files (restart without re-ingesting the kvstore): nbg_snapshot_save writes a finalized
 * engine's snapshot (schemas, dictionaries, CSR/CSC, columns, tag columns) to `path`;
 * nbg_snapshot_load replaces registration + loading + nbg_finalize on a fresh engine created with
 * the same num_parts / num_gpus / rank (a partitioned engine attaches its communicator first;
 * the load is then collective).  Schemas come from the file. */
int32_t nbg_snapshot_save(nbg_engine* e, const char* path);
int32_t nbg_snapshot_load(nbg_engine* e, const char* path);

typedef struct {
  uint64_t num_vertices;      /* vertices with at least one record in this rank's parts        */
  uint64_t num_edges;         /* live (latest-version) edge records, all signed types          */
  uint64_t device_bytes;      /* HBM held by the snapshot                                      */
  int32_t num_edge_types;     /* signed edge types present                                     */
  int32_t reserved;
  uint64_t tiny_queries;      /* GO queries run as one single-workgroup launch (tiny path)       */
  uint64_t host_agreements;   /* partitioned GO queries that agreed on rank-local statuses on the
                                 host before their first collective ($- / $var inputs); the others
                                 carry them in band                                              */
  uint64_t host_bytes;        /* host memory the finalized engine keeps beside its snapshot (row
                                 offsets, dictionary, the tiny path's walk bounds)               */
  uint64_t path_batch_contexts;  /* nbg_find_path_batch's contexts (rolling-run slots)          */
  uint64_t path_batch_reruns;    /* batched pairs whose search outgrew a context's lists and ran
                                    again on the engine's full-size one                          */
} nbg_stats;
int32_t nbg_get_stats(const nbg_engine* e, nbg_stats* out);

/* ---- GO N STEPS (GoExecutor semantics) ------------------------------------------------- */
/* Expression wire (WHERE / YIELD bytes here and the storage filter of nbg_gn_request): the bytes
 * of Expression::encode (src/common/filter/Expressions.cpp:93-98 and each class's encode), with
 * ONE extension.  The reference's TypeCastingExpression::encode writes nothing
 * (Expressions.cpp:801-802) and its decode throws (Expressions.h:830-832), so a cast cannot cross
 * the reference's own wire.  Here a cast is encoded as
 *     uint8 kind = 4 (kTypeCasting), uint8 ColumnType (0 INT, 1 STRING, 2 DOUBLE, 3 BIGINT,
 *     4 BOOL, 5 TIMESTAMP; Expressions.h:21-23), then the operand's own encoding,
 * which a graphd emits once its TypeCastingExpression::encode writes those three parts
 * (INTEGRATION.md §2 shows the body).  An UNPATCHED graphd drops the cast and its whole operand
 * from the bytes: the remaining tree is missing a subtree, so decoding runs out of bytes and
 * nbg_go fails with NBG_E_INVALID_ARGUMENT (nbg_get_neighbors: E_INVALID_FILTER for every part,
 * as the reference's processor answers a filter it cannot decode), never with rows.  A
 * cast at the ROOT of a WHERE encodes to zero bytes, which means "no WHERE" (where_len = 0): the
 * binding must reject a non-null filter_ whose encoding is empty.  Any other
 * ColumnType byte, or bytes left over after the tree, is NBG_E_INVALID_ARGUMENT. */
typedef struct {
  const int64_t* starts;          /* FROM vids; duplicates are kept (GoExecutor.cpp:136-195)  */
  uint64_t num_starts;
  const int32_t* edge_types;      /* OVER list, positive types, in order                      */
  int32_t num_edge_types;
  int32_t over_all;               /* OVER *: every registered positive edge type               */
  uint32_t steps;                 /* N >= 1                                                    */
  const uint8_t* where;           /* Expression::encode bytes of WHERE; NULL/0 = none         */
  uint32_t where_len;
  const uint8_t* const* yields;   /* Expression::encode bytes per YIELD column; 0 = default    */
  const uint32_t* yield_lens;     /*   (<edge>._dst per OVER edge, parser.yy:518-531)          */
  int32_t num_yields;
  int32_t distinct;               /* YIELD DISTINCT                                            */
  /* Piped / variable input for $-.col / $var.col in WHERE / YIELD: the rows the FROM $-.col or
   * $var.col came from, as columns.  GoExecutor::setupStarts indexes them by the FROM column
   * (input_vid_col; the last row of a vid wins, InterimResult.cpp:158-250) and a final-step row
   * reads the row of its source's root (VertexBackTracker, GoExecutor.h:169-188).  Column c holds
   * num_input_rows int64 payloads (int, double bits, bool 0/1) or, when input_kinds[c] is
   * NBG_V_STRING, a const char* const* of row strings.  num_input_cols = 0: no input. */
  int32_t num_input_cols;
  const char* const* input_names;
  const uint8_t* input_kinds;
  const void* const* input_cols;
  uint64_t num_input_rows;
  int32_t input_vid_col;
} nbg_go_request;

/* Rows are copied to host memory. */
int32_t nbg_go(nbg_engine* e, const nbg_go_request* req, nbg_rows** out);
/* Rows stay in HBM in the query workspace; nbg_rows_fetch() copies them to the host on demand.
 * They stay valid until nbg_rows_free: a later query that needs the workspace hands it over to
 * the live result (released by nbg_rows_free) and continues on a fresh one.  Every result must
 * be freed before nbg_destroy. */
int32_t nbg_go_device(nbg_engine* e, const nbg_go_request* req, nbg_rows** out);

/* ---- GO FROM $-.col / $var.col over a device-resident result (GoExecutor::setupStarts) ---------
 * `... | GO [N STEPS] FROM $-.col OVER ... [WHERE ...] [YIELD [DISTINCT] ...]' whose left side is a
 * result left in HBM by nbg_go_device, nbg_go_piped itself or any stage below: the start list and
 * the $- / $var input index are built on the device from the rows where they lie and handed to the
 * hop kernels of nbg_go (DESIGN.md "GO over device rows"); the host reads back one record of
 * counters.  `in` must be a device-resident result of this engine; it stays valid and unchanged.
 *
 * req is nbg_go's request.  Of its input fields, input_names names `in`'s columns, num_input_cols
 * must equal nbg_rows_num_cols(in) and input_vid_col is the FROM column; starts, num_starts,
 * input_kinds, input_cols and num_input_rows are ignored (the kinds are `in`'s own).  device != 0
 * leaves the rows in HBM as nbg_go_device does; otherwise they are copied to the host as by nbg_go.
 * The result is an ordinary nbg_rows: every accessor works on it and a device result feeds every
 * stage.
 *
 * For the same `in`, the rows (as a multiset), nbg_rows_step_stats, nbg_rows_edges_scanned and the
 * status are those of nbg_go / nbg_go_device with `starts' set to the fetched FROM column and
 * input_cols set to the fetched table, but for the device limits below:
 *   starts keep duplicates; a vid that is no vertex of the snapshot contributes nothing;
 *   under YIELD DISTINCT the starts are de-duplicated too (GoExecutor.cpp:101-107);
 *   the input index keeps the last row per vid, "last" by `in`'s fetch order (segment order;
 *   InterimResult.cpp:158-250);
 *   a final row reads the input row of its source's root; a root without one is an evaluation error.
 *
 * Statuses, in this order:
 *  1. NBG_E_INVALID_ARGUMENT: a null argument; `in` host-only or of another engine; input_names
 *     null (or one of its entries); num_input_cols != nbg_rows_num_cols(in); input_vid_col out of
 *     range; expression bytes that do not decode.
 *  2. NBG_E_UNSUPPORTED: a partitioned engine.
 *  3. Everything nbg_go_prepare answers for the statement, in its order, for an empty input too
 *     (prepare() runs before setupStarts).
 *  4. Zero input rows: NBG_OK and a zero-row result with the statement's columns (setupStarts
 *     returns before getVIDs, :371-375; then onEmptyInputs).
 *  5. NBG_E_EXECUTION_ERROR: the FROM column's kind is not INT, or its col_type is neither INT nor
 *     VID ("Column `x' not found": RowReader::getVid, RowReader.cpp:569-576, as nbg_fetch_vertices
 *     status 6).
 *  6. Device scope: see "Device limits" (NBG_E_UNSUPPORTED; the caller then fetches `in` and calls
 *     nbg_go with host inputs).
 *  7. From here on as nbg_go: its limits (the start list's entries plus edges under 2^32 - 1 among
 *     them), deferred name-resolution errors, evaluation errors, "Unknown Vertex".
 * A start list of at most 32 found entries is read back and takes nbg_go's short-list path.  Single
 * engine only; there is no prepared or asynchronous form. */
int32_t nbg_go_piped(nbg_engine* e, const nbg_rows* in, const nbg_go_request* req, int32_t device, nbg_rows** out);

/* Default YIELD of a GO without YIELD: the edge types whose `<edge>._dst` columns it returns, in
 * column order.  OVER e1, e2: the OVER order (parser.yy:518-531).  OVER * (over_all = 1, `over` =
 * every edge type as graphd requests them): the iteration order of the response's edge_schema map
 * (GoExecutor::getEdgeNamesFromResp, GoExecutor.cpp:481-499,546-561).  Returns the column count
 * (writes up to cap types) or a negative status. */
int32_t nbg_go_default_columns(nbg_engine* e, const int32_t* over, int32_t n, int32_t over_all, int32_t* out,
                               int32_t cap);

/* Prepared GO statement: GoExecutor::prepare() once (OVER / WHERE / YIELD validated and compiled
 * per OVER type, GoExecutor.cpp:136-263), then execute() from any number of start lists — the
 * request's starts are ignored by prepare.  Name-resolution errors stay deferred to the final step
 * as in nbg_go.  A statement belongs to its engine and must be freed before it. */
typedef struct nbg_go_stmt nbg_go_stmt;
int32_t nbg_go_prepare(nbg_engine* e, const nbg_go_request* req, nbg_go_stmt** out);
/* device != 0: rows stay in HBM as with nbg_go_device; otherwise as nbg_go. */
int32_t nbg_go_execute(nbg_go_stmt* stmt, const int64_t* starts, uint64_t num_starts, int32_t device,
                       nbg_rows** out);
void nbg_go_stmt_free(nbg_go_stmt* stmt);
/* The statement index.  A statement of at least two steps whose WHERE is `<edge column> <cmp>
 * <integer constant>` (either side; < <= > >= == !=) and whose YIELDs are `_dst` or constants
 * re-reads the WHERE column, and the `_dst` of the edges that fail, on every execution, while the
 * snapshot never changes.  Once the statement's completed executions have together scanned
 * NBG_STMT_INDEX_AFTER (default 0.25) times the OVER type's edge count in their final steps, the
 * next nbg_go_execute / nbg_go_submit builds, for the statement's first OVER type, the type's
 * adjacency restricted to the passing edges (4 bytes per vertex + 8 per passing edge of HBM, plus
 * 4 bytes per edge of the type while it is built) and the statement's later final steps over that
 * type copy rows from it (further OVER types keep the WHERE path).  Results,
 * nbg_rows_edges_scanned and nbg_rows_step_stats are unchanged; queries already in flight finish
 * as they were launched.  Not built: for nbg_go / nbg_go_device one-shots, on a partitioned
 * engine, while max_edge_returned_per_vertex is below the type's largest degree, when the index
 * with its build temporaries exceeds NBG_STMT_INDEX_MB (MiB; default: no limit) or half of the
 * free device memory, or when an allocation fails (never a query error).  NBG_STMT_INDEX=0
 * switches it off.  The three variables are read by nbg_go_prepare; NBG_STMT_INDEX_TRACE (any
 * value) logs each build and its duration on stderr.  nbg_go_stmt_free releases the index.
 * nbg_go_stmt_index_bytes: the HBM the statement's index holds (0: none). */
uint64_t nbg_go_stmt_index_bytes(const nbg_go_stmt* stmt);

/* Asynchronous execution (the way graphd runs concurrent queries): up to NBG_QUERY_SLOTS
 * (environment, default 6) queries of one engine in flight, each on its own workspace and HIP
 * stream.  nbg_go_submit enqueues the query and returns a ticket (when every slot is busy it first
 * completes the oldest query, whose result stays in its ticket); nbg_go_wait completes the ticket
 * (and every older one), returns its rows with nbg_go_execute's semantics and frees the ticket.
 * Device rows (device != 0) stay valid until nbg_rows_free, as with nbg_go_device (a slot whose
 * workspace still holds live rows gives it to them and takes a fresh one).  A ticket never
 * waited for is reclaimed by nbg_destroy; tickets must be
 * waited for before their statement is freed.  On a partitioned engine every rank must submit
 * the same queries in the same order (they are collectives).  Over RCCL each slot gets its own
 * communicator (split from the engine's, collectively, at the slot's first use; NBG_SLOT_COMMS=0
 * keeps one) and stream, so queries of different slots overlap on the device; the in-process
 * transport's slots share the engine's stream and communicator. */
typedef struct nbg_go_ticket nbg_go_ticket;
int32_t nbg_go_submit(nbg_go_stmt* stmt, const int64_t* starts, uint64_t num_starts, int32_t device,
                      nbg_go_ticket** out);
int32_t nbg_go_wait(nbg_go_ticket* ticket, nbg_rows** out);

int64_t nbg_rows_count(const nbg_rows* r);
int32_t nbg_rows_num_cols(const nbg_rows* r);
/* Σ_s E_s: adjacency entries scanned over all steps (the TEPS numerator); whole query, i.e.
 * summed over ranks on a partitioned engine. */
uint64_t nbg_rows_edges_scanned(const nbg_rows* r);
/* Per-step counters: frontier size |F_s| and edges E_s, s = 1..steps (arrays of length steps). */
int32_t nbg_rows_step_stats(const nbg_rows* r, uint64_t* frontier, uint64_t* edges, int32_t cap);
/* Rows into host memory: the device packs the row segments into contiguous columns and DMAs them
 * into pinned memory the engine reuses across results (returned by nbg_rows_free). */
int32_t nbg_rows_fetch(nbg_rows* r);
/* Host views (after nbg_go, or after nbg_rows_fetch): 8-byte cell payloads (int64, double bits,
 * bool as 0/1, string id) and value tags NBG_V_* per row.  The per-row tags are built on the first
 * nbg_rows_col_tags call; nbg_rows_col_kind gives a column's NBG_V_* kind when it is the same for
 * every row (the usual case: every OVER type yields the same kind), else -1. */
const int64_t* nbg_rows_col_bits(const nbg_rows* r, int32_t col);
const uint8_t* nbg_rows_col_tags(const nbg_rows* r, int32_t col);
int32_t nbg_rows_col_kind(const nbg_rows* r, int32_t col);
const char* nbg_rows_string(const nbg_rows* r, int64_t string_id);
/* Device view of a column's 8-byte payloads (valid for nbg_go_device results).  Rows are not
 * contiguous: each producing workgroup appends to its own region, so the result is the union of
 * the row ranges [begin, end) listed by nbg_rows_segment (host fetches pack them in that order). */
const void* nbg_rows_device_col(const nbg_rows* r, int32_t col);
int64_t nbg_rows_num_segments(const nbg_rows* r);
int32_t nbg_rows_segment(const nbg_rows* r, int64_t i, uint64_t* begin, uint64_t* end);
/* Order-independent digest of a result's rows, computed where the rows are (HBM for device
 * results): per row h = splitmix64(... splitmix64(0 ^ cell_0) ... ^ cell_{k-1}) over its 8-byte
 * cell payloads in column order; out[0] = rows, out[1] = XOR of h, out[2] = sum of h (mod 2^64).
 * Verifies results at sizes too large to fetch.  String cells hash their payload: the snapshot's
 * dictionary code for device rows (a string the query built — a concatenation, a cast to string —
 * is 1 << 62 | a 62-bit hash of its bytes, so equal strings hash alike), the result's string
 * index (nbg_rows_string) for host rows. */
int32_t nbg_rows_digest(const nbg_rows* r, uint64_t* out);
void nbg_rows_free(nbg_rows* r);

/* ---- GROUP BY over a device-resident GO result (GroupByExecutor semantics) ----------------
 * `| GROUP BY $-.x YIELD $-.x, COUNT(*), SUM($-.w) ...` over the rows a GO left in HBM, so a
 * caller need not fetch them to aggregate on the CPU (GroupByExecutor.cpp:226-322).
 * Input: a device-resident result of the same single engine (nbg_go_device, nbg_go_execute with
 * device = 1, nbg_go_wait); it stays valid and unchanged.  A host-only result is
 * NBG_E_INVALID_ARGUMENT.  Output: an ordinary device-resident nbg_rows of one segment, one row
 * per group; every nbg_rows_* accessor works on it and it spells its strings as `in` does
 * (dictionary codes, constants, derived codes).  The call runs under the engine lock on the
 * engine's stream; its scratch (tables, accumulators) is released before it returns.
 *
 * Zero input rows: NBG_OK and a zero-row result, with no check at all (execute() returns before
 * checkAll, GroupByExecutor.cpp:184-188).  Otherwise NBG_E_SYNTAX_ERROR (prepareYield,
 * prepareGroup, checkAll, :44-178) for: an empty group or yield list; a group column that is an
 * aggregate call (the request has no function field for group columns: a FunctionCall named like
 * an aggregate stands for it); "*" under anything but COUNT / COUNT_DISTINCT; a group column
 * that is neither `$-.name' of the input, nor a function call, nor a bare name (a string primary)
 * equal to the alias of a yield column that is itself `$-.name' (that column is then the key);
 * a yield `$-.name' absent from the input, or without a function and not among the `$-' group
 * keys; a `$var' yield.  A constant expression that fails to evaluate is
 * NBG_E_EXECUTION_ERROR.  Device scope: see "Device limits" (NBG_E_UNSUPPORTED; the caller then
 * runs the reference's loop over the fetched rows).
 *
 * Group identity: the key cells' payloads (the kinds are uniform per column).  Double keys -0.0
 * and 0.0 are one group (ColumnValue::operator==, std::hash<double>); which sign is reported is
 * unspecified.  NaN keys group by their bits — the reference makes every NaN row its own group.
 * Constant keys add nothing: with only constant keys there is one group.
 * Functions, by the input column's NBG_T_* type (constants carry their own kind):
 *   NONE   the key cell (or the constant);            COUNT  rows of the group (COUNT(*) alike)
 *   COUNT_DISTINCT  distinct payloads within the group (a constant: 1)
 *   SUM    INT / VID / TIMESTAMP: int64, wrapping, the column's type; DOUBLE: double; else INT 0
 *   AVG    INT: double(sum) / count; DOUBLE: sum / count; BOOL / STRING: 0.0
 *   MAX / MIN  the column's own order and type: signed int64, IEEE doubles, false < true,
 *          dictionary strings by their sorted-dictionary codes.  Doubles with NaNs: the
 *          reference's answer depends on its row order (a NaN never replaces a value and
 *          nothing replaces a leading NaN); here MAX / MIN reduce the IEEE total-order image
 *          of the bits, as ORDER BY sorts them, whatever the row order: a negative NaN is
 *          below -inf and a positive NaN above +inf, so the highest positive NaN of a group
 *          is its MAX and the lowest negative NaN its MIN.  Over zeros of both signs, which
 *          sign MAX / MIN report is unspecified (-0.0 == 0.0 in the reference's comparison)
 *          (tests/test_gpu_values_groupby.py pins both)
 *   STD    INT / DOUBLE: sqrt(sum((x - avg)^2) / n), DOUBLE; else INT 0
 *   BIT_AND / BIT_OR / BIT_XOR  INT columns and int constants; else INT 0
 * Result column kinds follow those rules (generateOutputSchema, :355-391).  Row order is
 * unspecified (the reference's is unordered_map iteration order).  A double SUM, AVG or STD adds
 * its terms in another order than the reference's row order, so it can differ in the last bits
 * (and between two calls); the final division and square root are IEEE-exact.
 * Single engine only: merging the ranks' rows of a partitioned engine is a later change. */
#define NBG_AGG_NONE           0   /* plain column */
#define NBG_AGG_COUNT          1
#define NBG_AGG_COUNT_DISTINCT 2
#define NBG_AGG_SUM            3
#define NBG_AGG_AVG            4
#define NBG_AGG_MAX            5
#define NBG_AGG_MIN            6
#define NBG_AGG_STD            7
#define NBG_AGG_BIT_AND        8
#define NBG_AGG_BIT_OR         9
#define NBG_AGG_BIT_XOR        10
typedef struct {
  const char* const* input_names;        /* names of `in`'s columns (nbg_rows carries none)      */
  const uint8_t* const* group_exprs;     /* Expression::encode bytes per GROUP BY column          */
  const uint32_t* group_lens;
  int32_t num_groups;
  const uint8_t* const* yield_exprs;     /* ... per YIELD column (COUNT(*): the string primary "*") */
  const uint32_t* yield_lens;
  const int32_t* yield_funs;             /* NBG_AGG_* per YIELD column                             */
  const char* const* yield_aliases;      /* AS name or NULL (the array itself may be NULL)         */
  int32_t num_yields;
} nbg_group_request;
int32_t nbg_group_by(nbg_engine* e, const nbg_rows* in, const nbg_group_request* req, nbg_rows** out);

/* ---- ORDER BY / LIMIT over a device-resident result (OrderByExecutor, LimitExecutor) -------
 * `| ORDER BY $-.x [ASC|DESC], ... | LIMIT [offset,] count` over rows in HBM, either clause alone
 * or both fused (grammar: parser.yy:727-767; every factor is an InputPropertyExpression, so its
 * name is all there is to pass).  Input and output follow nbg_group_by's contract: `in` is a
 * device-resident result of the same single engine (a GO result, the output of nbg_group_by or of
 * nbg_order_by itself); it stays valid and unchanged.  A host-only result, or one of another
 * engine, is NBG_E_INVALID_ARGUMENT.  `out` is an ordinary device-resident nbg_rows of one
 * segment whose row order (nbg_rows_fetch, the device view) is the result order; it has `in`'s
 * columns, kinds, col_types, string constants and derived-string table, every nbg_rows_*
 * accessor works on it and it can be fed to nbg_group_by.  The call runs under the engine lock
 * on the engine's stream; its scratch (keys, permutations, candidates) is released before it
 * returns.  A failed allocation is NBG_E_OUT_OF_MEMORY.
 *
 * Statuses, in this order: has_limit with offset < 0 or count < 0 is NBG_E_SYNTAX_ERROR
 * (LimitExecutor::prepare, LimitExecutor.cpp:18-28), even for an empty input.  Zero input rows:
 * NBG_OK and a zero-row result with no factor check (OrderByExecutor::beforeExecute returns
 * before it, OrderByExecutor.cpp:137-139).  Otherwise a factor name absent from input_names is
 * NBG_E_EXECUTION_ERROR (OrderByExecutor.cpp:140-152, OrderByTest.WrongFactor); with duplicate
 * column names the first match wins (getFieldIndex).  Device scope: see "Device limits"
 * (NBG_E_UNSUPPORTED; the caller then sorts the fetched rows as the reference does).
 * LIMIT (LimitExecutor.cpp:30-66): count == 0 or rows <= offset give zero rows; otherwise the
 * result is rows [offset, min(rows, offset + count)) of the ordered input (offset + count
 * saturates instead of overflowing).
 *
 * Order (OrderByExecutor.cpp:94-131): ColumnValue::operator< per factor, later factors breaking
 * the ties operator== leaves: signed int64 for INT / VID / TIMESTAMP; IEEE order for DOUBLE, where
 * -0.0 and 0.0 are equal (they do not decide, the next factor does); false < true; strings by
 * bytes — dictionary strings by their codes, which are 2 * index in the dictionary sorted by
 * std::string::operator<, i.e. by unsigned bytes (negative codes are dictionary codes too and sort
 * first).  DESC reverses a factor.  Rows equal under every factor come in unspecified order, and
 * with a LIMIT which of them fall inside the window is unspecified (the reference's std::sort is
 * not stable).  NaN factors are unspecified in the reference (they break its comparator); here
 * they sort by their bits' IEEE total-order image.
 * Without factors (LIMIT only) the order is the input's own segment order, the order
 * nbg_rows_fetch delivers: limit(in, off, n) fetches exactly in's fetched rows [off, off + n).
 * Single engine only: merging the ranks' orders of a partitioned engine is a later change. */
typedef struct {
  const char* const* input_names;   /* names of `in`'s columns, as in nbg_group_request          */
  const char* const* factor_names;  /* ORDER BY factors: the `name' of `$-.name' (or bare label) */
  const uint8_t* factor_desc;       /* per factor: 0 ASC, 1 DESC                                 */
  int32_t num_factors;              /* 0: no ORDER BY clause (LIMIT only)                        */
  int32_t has_limit;                /* 0: no LIMIT clause                                        */
  int64_t offset, count;            /* LIMIT offset, count                                       */
} nbg_order_request;
int32_t nbg_order_by(nbg_engine* e, const nbg_rows* in, const nbg_order_request* req, nbg_rows** out);

/* ---- UNION / INTERSECT / MINUS over two device-resident results (SetExecutor) ---------------
 * `left UNION [ALL|DISTINCT] right`, `left INTERSECT right`, `left MINUS right` over rows in HBM
 * (SetExecutor.cpp:98-383; grammar: parser.yy:1109-1141).  Inputs and output follow nbg_group_by's
 * and nbg_order_by's contract: `left` and `right` are device-resident results of the same single
 * engine (GO results, or outputs of nbg_group_by, nbg_order_by or nbg_set_op); left == right is
 * allowed; both stay valid and unchanged.  `out` is an ordinary device-resident nbg_rows of one
 * segment in a workspace of its own: every nbg_rows_* accessor works on it and it feeds
 * nbg_group_by, nbg_order_by and nbg_set_op.  It carries no column names: the caller keeps the
 * left operand's (SetExecutor.cpp:129).  The call runs under the engine lock on the engine's
 * stream; its scratch (12 bytes per slot of a row table of twice the inserted rows, one flag byte
 * per row, 24 bytes per chunk of 2,048 rows) is released before it returns.  A failed allocation
 * is NBG_E_OUT_OF_MEMORY.
 *
 * Statuses, in this order:
 *  1. NBG_E_INVALID_ARGUMENT: a null argument, `op` outside 1..3, rows of another engine, a
 *     host-only result.
 *  2. NBG_E_UNSUPPORTED: a partitioned engine.
 *  3. NBG_E_EXECUTION_ERROR ("Field count not match."): different column counts, even when both
 *     inputs are empty (:131-136, SetTest.ExecutionError).
 *  4. The empty-input shortcuts, before any schema or cast check (:137-141, :163-174, :273-277,
 *     :327-337): both empty: zero rows.  UNION with one side empty: the other side as it is, with
 *     its own column types and not de-duplicated, even under DISTINCT.  INTERSECT with either side
 *     empty, MINUS with the left empty: zero rows.  MINUS with the right empty: the left as it is.
 *     "As it is" is exactly what nbg_order_by returns for that side with no factors and no LIMIT,
 *     its NBG_E_UNSUPPORTED cases included.
 *  5. Device scope: see "Device limits" (NBG_E_UNSUPPORTED; the caller then runs the reference's
 *     loop over the fetched rows).  The two inputs' derived-string tables are merged on the host;
 *     one derived code standing for two texts is NBG_E_EXECUTION_ERROR ("derived-string hash
 *     collision").
 *
 * Implicit casts (checkSchema / doCasting, :219-262; InterimResult::castTo*, InterimResult.cpp:
 * 292-538): column c's type is its col_type, or its kind's natural type when unset.  Where the two
 * sides' types differ, every right cell is cast to the left's type, in all three operators and
 * before any comparison; the result takes the left's kinds, types and string spelling.
 *   INT / VID / TIMESTAMP among each other: the payload is unchanged.
 *   DOUBLE to integer-like: truncation toward zero (NaN and |x| >= 2^63 are undefined in the
 *   reference and unspecified here).  BOOL to integer-like: 0 / 1.
 *   integer-like to DOUBLE: (double), round to nearest even.  BOOL to DOUBLE: 0.0 / 1.0.
 *   integer-like to BOOL: != 0.  DOUBLE to BOOL: != 0.0 (NaN is true, -0.0 is false).
 * A result row that came from the right holds the cast value.
 *
 * Row equality, after the cast and with the left's types: payload equality for integer-like, BOOL
 * and string codes (dictionary codes and derived codes are engine-wide, so they compare across
 * results); IEEE == for DOUBLE: -0.0 equals 0.0, and which sign a surviving row reports is
 * unspecified.  A NaN cell equals nothing in INTERSECT and MINUS, as in the reference: such a left
 * row never appears in an INTERSECT and always survives a MINUS.  In UNION DISTINCT the reference's
 * sort comparator is undefined on NaN; here NaNs are equal by their bits, as in GROUP BY keys.
 *
 * Multiplicities, for a row value occurring cL times on the left and cR times on the right:
 *   UNION ALL                cL + cR                (:208-210)
 *   UNION / UNION DISTINCT   1                      (doDistinct, :265-269)
 *   INTERSECT                min(cL, cR)            (:311-319: the reference moves the matched right
 *                            row out of its vector; the moved-from row has no columns and matches
 *                            nothing again, so every right row is used up by one left row)
 *   MINUS                    cL if cR == 0, else 0  (:371-379)
 * Row order: UNION ALL is the left's fetch order followed by the right's, so
 * limit(union_all(a, b)) is exact like LIMIT-only nbg_order_by.  The other operators' order is
 * unspecified (the reference's is the left's, or sorted for DISTINCT, but the left's own segment
 * order is already not the reference's): pipe into nbg_order_by for an order.
 * Single engine only: merging the ranks' rows of a partitioned engine is a later change. */
#define NBG_SET_UNION     1
#define NBG_SET_INTERSECT 2
#define NBG_SET_MINUS     3
typedef struct {
  int32_t op;        /* NBG_SET_* */
  int32_t distinct;  /* UNION only: 0 = UNION ALL, else UNION / UNION DISTINCT; ignored otherwise */
} nbg_set_request;
int32_t nbg_set_op(nbg_engine* e, const nbg_rows* left, const nbg_rows* right, const nbg_set_request* req,
                   nbg_rows** out);

/* ---- piped YIELD ... WHERE over a device-resident result (YieldExecutor) ---------------------
 * `| YIELD $-.d AS id, $-.w * 2 AS w2 WHERE $-.w > 50` over rows in HBM
 * (YieldExecutor::executeInputs, YieldExecutor.cpp:178-282; grammar: parser.yy:707-713; a YIELD
 * sentence has no DISTINCT).  Input and output follow nbg_order_by's contract: `in` is a
 * device-resident result of the same single engine (a GO result, or the output of nbg_group_by,
 * nbg_order_by, nbg_set_op or nbg_yield itself); it stays valid and unchanged.  A host-only result,
 * or one of another engine, is NBG_E_INVALID_ARGUMENT.  `out` is an ordinary device-resident
 * nbg_rows of one segment in a workspace of its own: every nbg_rows_* accessor works on it and it
 * feeds nbg_group_by, nbg_order_by, nbg_set_op and nbg_yield.  It carries no column names (the
 * caller keeps the YIELD aliases).  The call runs under the engine lock on the engine's stream; its
 * scratch (one flag byte per row, 32 bytes per chunk of 2,048 rows, the compiled program) is
 * released before it returns.  A failed allocation is NBG_E_OUT_OF_MEMORY.
 *
 * Row order: the input's fetch order (segment order) with the failing rows removed, as the
 * reference delivers it.  So `ORDER BY | YIELD | LIMIT` and `YIELD | LIMIT` are exact.
 *
 * Statuses, in this order:
 *  1. NBG_E_INVALID_ARGUMENT: a null argument, num_yields < 1, a host-only or foreign `in`,
 *     expression bytes that do not decode (nbg_go's rules, the cast wire extension included).
 *  2. NBG_E_UNSUPPORTED: a partitioned engine.
 *  3. NBG_E_SYNTAX_ERROR: any `$^', `$$' or edge-property node in WHERE or a YIELD (syntaxCheck,
 *     :116-122; YieldTest.error); some yield_funs[i] != NBG_AGG_NONE together with a column that is
 *     a bare `$-.x' / `$var.x' without a function (checkAggFun, :33-58; YieldTest.AggCall).
 *  4. NBG_E_EXECUTION_ERROR: both `$-' and `$var' referenced, or more than one variable name
 *     (:124-135).
 *  5. Zero input rows: NBG_OK and a zero-row result with one column per YIELD after `$-.*'
 *     expansion.  Whether unknown column names are diagnosed here is unspecified (the reference
 *     dereferences a null schema).
 *  6. A `$-.name' / `$var.name' absent from input_names: NBG_E_EXECUTION_ERROR ("column `x' not
 *     exist in input.", :298-316; YieldTest.error).  With duplicate names the first match wins.
 *  7. Device scope: see "Device limits" (NBG_E_UNSUPPORTED; the caller then runs the reference's
 *     loop over the fetched rows).
 *  8. Evaluation (NBG_E_EXECUTION_ERROR, no result): per row the WHERE is evaluated first, through
 *     Expression::asBool, and the YIELDs only on the rows that pass.  An evaluation error in the
 *     WHERE of any row, or in a YIELD of a passing row, fails the call.  A YIELD error on a row the
 *     WHERE rejects is not an error.  (The reference's first-row schema probe, :318-340, evaluates
 *     the first row's YIELDs unfiltered and reads past its record when that fails: undefined
 *     there, unspecified here.)
 *
 * Expressions: a YIELD column that is exactly `$-.*' or `$var.*' expands to every input column in
 * order (YieldClauseWrapper::prepare).  Everything nbg_go's compiler accepts over `$-' columns and
 * constants is accepted with the same results: arithmetic, relational and logical operators, unary
 * operators, casts between INT / DOUBLE / BOOL / TIMESTAMP, hash, the math functions, udf_is_in,
 * comparisons of dictionary strings, now() and rand*().  `$var.x' reads the same `in' as `$-.x'.
 * A request that references no `$-' / `$var' column at all is the reference's executeConstant (one
 * row, whatever the input): the binding answers it without this call, which evaluates per row.
 *
 * Result schema: a column's kind is the compiler's static kind (input kinds are uniform per
 * column, so this is the reference's "kind of the first row's value").  col_types follow
 * Collector::getSchema (TraverseExecutor.cpp:163-203): the kind's own type (INT for every integer
 * payload, so a VID or TIMESTAMP column passed through becomes INT), or, for a cast at the root of
 * the YIELD, the cast's type; nbg_set_op's implicit casts read these types.  A constant YIELD is a
 * constant column.  String constants outside the dictionary and the input's derived-string table
 * are carried over, as nbg_order_by carries them.
 * Single engine only.  yield_funs exists so that whole-input aggregates (a later change) do not
 * alter the struct. */
typedef struct {
  const char* const* input_names;    /* names of `in`'s columns, as in nbg_group_request        */
  const uint8_t* where;              /* Expression::encode bytes of WHERE; NULL/0 = none         */
  uint32_t where_len;
  const uint8_t* const* yield_exprs; /* Expression::encode bytes per YIELD column                */
  const uint32_t* yield_lens;
  const int32_t* yield_funs;         /* NBG_AGG_* per column, or NULL (all NBG_AGG_NONE)         */
  int32_t num_yields;
} nbg_yield_request;
int32_t nbg_yield(nbg_engine* e, const nbg_rows* in, const nbg_yield_request* req, nbg_rows** out);

/* ---- piped YIELD with aggregate functions and no GROUP BY (YieldExecutor) ----------------------
 * `| YIELD AVG($-.age), SUM($-.like), COUNT(*), 1+1` and
 * `| YIELD COUNT(*), SUM($-.w * 2 + 1), MAX($-.w) WHERE $-.w < 50` over rows in HBM
 * (YieldExecutor::checkAggFun / executeInputs, YieldExecutor.cpp:33-58, 178-282; the functions:
 * AggregateFunction.h; YieldTest.AggCall).  The request is nbg_yield's struct with at least one
 * yield_funs[i] != NBG_AGG_NONE; nbg_yield itself keeps answering such a request with
 * NBG_E_UNSUPPORTED.  A request that references no `$-' / `$var' column at all is the reference's
 * executeConstant / AggregateConstant: the binding answers it without this call.
 *
 * Input and output follow nbg_yield's contract: `in` is a device-resident result of the same
 * single engine; it stays valid and unchanged.  `out` is an ordinary device-resident nbg_rows of
 * one segment and ONE ROW in a workspace of its own, usable by every nbg_rows_* accessor and every
 * stage.  The call runs under the engine lock on the engine's stream; its scratch (8 bytes per
 * accumulator slot and 4 bytes per chunk of 2,048 rows, the compiled program; for each
 * COUNT_DISTINCT over a column or an expression additionally nbg_yield's scratch, the argument of
 * the kept rows as a one-column result, and nbg_set_op's scratch for its UNION DISTINCT) is
 * released before it returns.  A failed allocation is NBG_E_OUT_OF_MEMORY.
 *
 * Statuses, in this order:
 *  1. NBG_E_INVALID_ARGUMENT: nbg_yield's cases; a null yield_funs, or no yield_funs[i] !=
 *     NBG_AGG_NONE at all (that request is nbg_yield's); a function outside
 *     NBG_AGG_NONE..NBG_AGG_BIT_XOR.
 *  2. NBG_E_UNSUPPORTED: a partitioned engine.
 *  3. NBG_E_SYNTAX_ERROR: any `$^', `$$' or edge-property node (syntaxCheck, :116-122); a column
 *     that is a bare `$-.x' / `$var.x' (after `$-.*' expansion) without a function (checkAggFun,
 *     :33-58; YieldTest.AggCall).
 *  4. NBG_E_EXECUTION_ERROR: both `$-' and `$var' referenced, or more than one variable name.
 *  5. Zero input rows: NBG_OK and a zero-row result with one column per YIELD (nbg_yield's status
 *     5: the reference dereferences a null schema there, so it stays unspecified).
 *  6. A referenced column absent from input_names: NBG_E_EXECUTION_ERROR, with nbg_yield's
 *     messages.  With duplicate names the first match wins.
 *  7. Device scope: see "Device limits" (NBG_E_UNSUPPORTED).
 *  8. Evaluation (NBG_E_EXECUTION_ERROR, no result): per row the WHERE is evaluated first and the
 *     arguments only on the rows that pass.  An evaluation error in the WHERE of any row, or in an
 *     argument on a passing row, fails the call.  An argument error on a row the WHERE rejects is
 *     not an error.
 *  9. The WHERE rejects every row of a non-empty input and the statement has a MAX, a MIN or a
 *     column without a function: NBG_E_EXECUTION_ERROR ("Not Support: 0": a fresh function object
 *     holds an empty ColumnValue, which InterimResult::getResultWriter refuses,
 *     InterimResult.cpp:602-640).
 *
 * Value types (they differ from nbg_group_by's): the type a function sees is the one
 * getOutputSchema gives the column (Collector::getSchema, TraverseExecutor.cpp:163-203): the static
 * kind's own type (INT for every integer payload, so a VID or TIMESTAMP column reads as INT and
 * AVG($-.d) over a VID column is defined here), or, for a cast at the root of the argument, the
 * cast's type.  The only TIMESTAMP-typed argument is therefore a root `(timestamp)' cast.
 *
 * Functions (AggregateFunction.h), over the n >= 1 kept rows:
 *   none            a column without a function and without `$-': the value (Group::apply keeps
 *                   the last row's); on the device only a constant-foldable one; the constant's kind
 *   COUNT           n, INT, for any argument, `*' included
 *   COUNT_DISTINCT  the number of distinct values, INT; -0.0 and 0.0 are one value (ColumnValue ==,
 *                   std::hash<double>); NaNs count by their bits: equal bits are one value (the
 *                   reference counts every NaN row, no NaN being equal to itself); a constant or `*': 1
 *   SUM             INT / TIMESTAMP: wrapping int64 of that type; DOUBLE: double; BOOL / STRING: INT 0
 *   AVG             INT: double(wrapped sum) / n; DOUBLE: sum / n; BOOL / STRING: 0.0; TIMESTAMP: a
 *                   device limit
 *   MAX / MIN       the argument's type and order, exactly as nbg_group_by documents them: signed
 *                   int64; doubles by the IEEE total-order image, NaNs included, either sign over
 *                   zeros; false < true; dictionary strings by code
 *   STD             INT / DOUBLE: sqrt(sum((x - avg)^2) / n), DOUBLE; anything else (TIMESTAMP
 *                   included: Stdev::apply collects nothing): INT 0
 *   BIT_AND / BIT_OR / BIT_XOR   INT-typed arguments only; anything else: INT 0
 * col_types are the result value's type (schema->appendCol(name, val.getType()), :260-278).
 * Arguments whose expressions are equal share one evaluation and their accumulators.
 *
 * The WHERE rejects every row of a non-empty input: one row of each fresh function object's
 * getResult: COUNT and COUNT_DISTINCT 0; SUM INT 0, whatever the argument's type; STD and BIT_* INT
 * 0; AVG a DOUBLE NaN (0.0 / 0; payload and sign unspecified).  With a MAX, a MIN or a column
 * without a function it is status 9.  So the result's kinds are decided after the kept count is
 * known.
 *
 * Repeatability: a chunk's partial results depend on its rows alone, and they are folded in an
 * order the number of chunks alone decides, whatever the grid and the scheduling: two calls on the
 * same nbg_rows give bit-identical doubles.  The same rows in another segmentation (after an
 * nbg_order_by, say) may differ in the last bits of a double SUM / AVG / STD.
 * Single engine only. */
int32_t nbg_yield_agg(nbg_engine* e, const nbg_rows* in, const nbg_yield_request* req, nbg_rows** out);

/* ---- piped FETCH PROP ON <tag> over a device-resident result (FetchVerticesExecutor) ----------
 * `| FETCH PROP ON player $-.id YIELD player.name, player.age` over rows in HBM
 * (FetchVerticesExecutor.cpp:19-311, FetchExecutor.cpp:14-131).  Input and output follow
 * nbg_yield's contract: `in` is a device-resident result of the same single engine (a GO result,
 * or the output of nbg_group_by, nbg_order_by, nbg_set_op, nbg_yield or nbg_fetch_vertices itself);
 * it stays valid and unchanged.  `out` is an ordinary device-resident nbg_rows of one segment in a
 * workspace of its own: every nbg_rows_* accessor works on it and it feeds nbg_group_by,
 * nbg_order_by, nbg_set_op, nbg_yield and nbg_fetch_vertices.  It carries no column names.  The
 * call runs under the engine lock on the engine's stream; its scratch is released before it
 * returns: 5 bytes per input row (a 4-byte dense id and a keep byte), 32 bytes per chunk of at most
 * 2,048 rows (the 24-byte chunk list entry, a count and a base), a 16-byte state word pair and the
 * compiled program; a literal vid list adds its temporary input of 8 bytes per vid, and `distinct`
 * adds nbg_set_op's UNION DISTINCT scratch beside the rows not yet de-duplicated.  A failed
 * allocation is NBG_E_OUT_OF_MEMORY.  With in == NULL the evaluated vid list `vids` of
 * `FETCH PROP ON t 1, 2` is uploaded into a temporary one-column result and takes the same path.
 *
 * Rows: one result row per input row whose vid is found; duplicates are kept (getVIDs keeps them,
 * InterimResult.cpp:29-49, and the storage client sends every occurrence).  A vid is found when it
 * is a vertex of the snapshot, the vertex carries a decoded record of the tag, and that record lives
 * in the part the storage client asks, uint64(vid) % num_parts + 1 (StorageClient::getVertexProps;
 * QueryBoundProcessor::processVertex).  A live record whose value does not decode is no record
 * here: collectProps skips every bad value (QueryBaseProcessor.inl:323-326), so no tag_data is
 * sent, as nbg_get_neighbors has it.  A vid that is absent, without the tag, undecodable or
 * invisible yields no row and no error (FetchVerticesTest.nonExistVertex; processResult skips empty tag_data,
 * FetchVerticesExecutor.cpp:179-181).
 *
 * Row order: the input's fetch order with the missing rows removed (the reference's order is per
 * host and part, hence unspecified), so `ORDER BY | FETCH | LIMIT` is exact.  Under `distinct`
 * the order is unspecified.
 *
 * distinct (YIELD DISTINCT): the result holds each distinct output row once (processResult's
 * uniqResult, :159, :221-228); doubles compare as in nbg_set_op.  De-duplicating the vids first
 * (getDistinctVIDs, InterimResult.cpp:51-72; setupVidsFromExpr, :246-283) is then redundant.
 *
 * Expressions: `tag.prop' (an alias property whose alias is the tag's registered name) reads the
 * found vertex's column; everything nbg_yield accepts over columns and constants is accepted with
 * the same results.  A YIELD that is exactly `tag.prop' is copied without the interpreter.
 *
 * Result schema: col_types follow FetchExecutor::prepareYield (FetchExecutor.cpp:35-47): a bare
 * `tag.prop' takes the tag schema's field type, a root cast the cast's type, anything else the
 * value's natural type.  String cells are dictionary codes; string constants outside the
 * dictionary are carried as nbg_yield carries them.
 *
 * Statuses, in this order:
 *  1. NBG_E_INVALID_ARGUMENT: a null argument; `in` host-only or of another engine; in == NULL
 *     with vids == NULL and num_vids > 0; expression bytes that do not decode.
 *  2. NBG_E_UNSUPPORTED: a partitioned engine.
 *  3. NBG_E_EXECUTION_ERROR: tag_id not registered ("tag schema not exist", :45-50); vid_col
 *     equal to `*' (:79-81).
 *  4. NBG_E_SYNTAX_ERROR, for an empty input too (prepareYield runs before setupVids): any `$^' /
 *     `$$' node; any `$-' / `$var' node in a YIELD; an alias other than the tag's name
 *     (FetchExecutor.cpp:50-68).
 *  5. Zero input rows: NBG_OK and a zero-row result with one column per YIELD (onEmptyInputs,
 *     FetchExecutor.cpp:99-107).
 *  6. NBG_E_EXECUTION_ERROR: vid_col absent from input_names, or a column whose kind is not INT
 *     or whose col_type is neither INT nor VID ("Column `x' not found": RowReader::getVid,
 *     RowReader.cpp:569-576, refuses TIMESTAMP, DOUBLE, BOOL and STRING); no `tag.prop' anywhere
 *     in the YIELDs ("No props declared.", :110-115); a prop the tag's latest schema lacks ("Get
 *     props failed", :121-124).
 *  7. Device scope: see "Device limits" (NBG_E_UNSUPPORTED; the caller then fetches the ids and
 *     runs the reference's path).
 *  8. An evaluation error in a YIELD of a found row: NBG_E_EXECUTION_ERROR, no result (:206-210).
 * Single engine only.  The join is a binary search of the sorted vid table per row (DESIGN.md
 * "FETCH PROP over device rows"). */
typedef struct {
  const char* const* input_names;    /* names of `in`'s columns; unused when in == NULL            */
  const char* vid_col;               /* the `name' of `$-.name' / `$var.name'; unused when in == NULL */
  const int64_t* vids;               /* in == NULL: the evaluated vid list of `FETCH PROP ON t 1, 2' */
  uint64_t num_vids;
  int32_t tag_id;                    /* the tag of `ON <tag>' (the binding resolved the name)       */
  const uint8_t* const* yield_exprs; /* Expression::encode bytes per YIELD column                   */
  const uint32_t* yield_lens;
  int32_t num_yields;                /* 0: no YIELD clause: every column of the tag's latest schema,
                                        in schema order (FetchExecutor::setupColumns)               */
  int32_t distinct;                  /* YIELD DISTINCT                                              */
} nbg_fetch_request;
int32_t nbg_fetch_vertices(nbg_engine* e, const nbg_rows* in, const nbg_fetch_request* req, nbg_rows** out);

/* ---- piped FETCH PROP ON <edge> over a device-resident result (FetchEdgesExecutor) -------------
 * `| FETCH PROP ON serve $-.src->$-.dst[@$-.rank] YIELD serve.start_year` over rows in HBM, and
 * `FETCH PROP ON serve 100->200@0, 100->201` (FetchEdgesExecutor.cpp:17-384, FetchExecutor.cpp:14-131,
 * QueryEdgePropsProcessor.cpp:17-101).  Input and output follow nbg_fetch_vertices' contract: `in`
 * is a device-resident result of the same single engine (a GO result, or the output of nbg_group_by,
 * nbg_order_by, nbg_set_op, nbg_yield, nbg_fetch_vertices or nbg_fetch_edges itself); it stays valid
 * and unchanged.  `out` is an ordinary device-resident nbg_rows of one segment in a workspace of its
 * own: every nbg_rows_* accessor works on it and it feeds every stage, nbg_fetch_vertices and
 * nbg_fetch_edges too.  It carries no column names.  The call runs under the engine lock on the
 * engine's stream; its scratch is released before it returns: 5 bytes per input row (a 4-byte edge
 * index and a keep byte; 9 when a YIELD reads `_src', which keeps the source's 4-byte dense id), 32
 * bytes per chunk of at most 2,048 rows (the 24-byte chunk list entry, a count and a base), a
 * 16-byte state word pair and the compiled program; literal keys add their temporary input of 24
 * bytes per key, and `distinct' adds nbg_set_op's UNION DISTINCT scratch beside the rows not yet
 * de-duplicated.  A failed allocation is NBG_E_OUT_OF_MEMORY.  With in == NULL the evaluated keys
 * `srcs' / `dsts' / `ranks' are uploaded into a temporary three-column result and take the same path.
 *
 * Rows: one result row per input row whose key is found; duplicates are kept (setupEdgeKeysFromRef
 * keeps them without DISTINCT, :182-197).  A key (src, dst, rank) is found when src is a vertex of
 * the snapshot, that vertex lives in the part the storage client asks (StorageClient::getEdgeProps
 * clusters the keys by src: uint64(src) % num_parts + 1), and src's out-edges of the type hold an
 * entry with that (rank, dst).  The latest version answers (collectEdgesProps takes the first key of
 * the prefix scan, the newest write, :22-38); older versions are never read, and
 * max_edge_returned_per_vertex does not apply (QueryEdgePropsProcessor has no cap).  A key that is
 * not found yields no row and no error (FetchEdgesTest.nonExistEdge); when nothing is found the
 * result is NBG_OK with zero rows.  rank_col == NULL (in == NULL: ranks == NULL) gives every key
 * rank 0 (:187).
 *
 * Row order: the input's fetch order with the missing rows removed (the reference's order is per
 * host and part, hence unspecified), so `ORDER BY | FETCH | LIMIT' is exact.  Under `distinct'
 * the order is unspecified.
 *
 * distinct (YIELD DISTINCT): the result holds each distinct output row once (processResult's
 * uniqResult, :322, :371-375); doubles compare as in nbg_set_op.  De-duplicating the keys first
 * (EdgeKeyHashSet, :178-197, :204-255) is then redundant.
 *
 * Expressions: everything nbg_go's compiler accepts for one OVER type over the edge's props,
 * `_src', `_dst', `_rank', `_type' and constants, with GO's results (`edge._type' is the edge's
 * name, a STRING, as EdgeTypeExpression::eval has it).  A YIELD that is exactly `edge.prop' is
 * copied without the interpreter; a constant YIELD is a kernel argument.
 * Unspecified in the reference: an edge whose value does not decode.  There collectProps writes a
 * short row the executor then misreads.  Here a YIELD that reads a schema prop of such an edge is an
 * evaluation error (status 8); `_src', `_dst', `_rank' and `_type' of it still evaluate.
 *
 * Result schema: col_types follow FetchExecutor::prepareYield (FetchExecutor.cpp:35-47): a bare
 * `edge.prop' takes the edge schema's field type, a root cast the cast's type, anything else the
 * value's natural type.  `_src', `_dst', `_rank' and `_type' are no alias expressions there
 * (Expression::isAliasExpression is kind_ == kAliasProp, Expressions.h:192-194; they have kinds of
 * their own), and an edge schema has no field of those names, so they take the natural type: INT
 * for the first three, STRING for `_type'.  String cells are dictionary codes; string constants
 * outside the dictionary are carried as nbg_yield carries them.
 *
 * Statuses, in this order:
 *  1. NBG_E_INVALID_ARGUMENT: a null argument; `in' host-only or of another engine; in != NULL
 *     with a null src_col or dst_col; in == NULL with num_keys > 0 and null srcs or dsts;
 *     expression bytes that do not decode.
 *  2. NBG_E_UNSUPPORTED: a partitioned engine.
 *  3. NBG_E_EXECUTION_ERROR: edge_type not registered ("edge schema not exist", :36-47); src_col,
 *     dst_col or rank_col equal to `*' (:83-88).
 *  4. NBG_E_SYNTAX_ERROR, for an empty input too (prepareYield runs before setupEdgeKeys): any `$^' /
 *     `$$' node; any `$-' / `$var' node in a YIELD; an alias other than the edge's name
 *     (FetchExecutor.cpp:50-68; FetchEdgesTest.syntaxError).  ("Only support single data source.",
 *     EdgeKeyRef::varname, is the binding's to answer: the request carries column names only.)
 *  5. Zero input rows or zero keys: NBG_OK and a zero-row result with one column per YIELD
 *     (onEmptyInputs, FetchExecutor.cpp:99-107).
 *  6. NBG_E_EXECUTION_ERROR: src_col, dst_col or rank_col (in that order) absent from
 *     input_names, or a column whose kind is not INT or whose col_type is neither INT nor VID
 *     ("Column `x' not found": getVIDs -> RowReader::getVid, which the rank column goes through
 *     too, :158-176); no alias property anywhere in the YIELDs ("No props declared.", :270-274);
 *     a prop the edge's latest schema lacks ("Get props failed", :280-283).
 *  7. Device scope: see "Device limits" (NBG_E_UNSUPPORTED; the caller then fetches the keys and
 *     runs the reference's path).
 *  8. An evaluation error in a YIELD of a found row: NBG_E_EXECUTION_ERROR, no result (:355-359).
 * Single engine only.  The join is a binary search of the sorted vid table per row, then one of
 * the source's CSR row in the key's byte order (DESIGN.md "FETCH PROP ON <edge> over device rows"). */
typedef struct {
  const char* const* input_names;    /* names of `in`'s columns; unused when in == NULL             */
  const char* src_col;               /* the `name' of `$-.name' / `$var.name' left of `->'          */
  const char* dst_col;               /* ... right of `->'                                            */
  const char* rank_col;              /* ... after `@'; NULL: no rank given, every key has rank 0     */
  const int64_t* srcs;               /* in == NULL: the evaluated keys of `FETCH PROP ON e 1->2@0,..' */
  const int64_t* dsts;
  const int64_t* ranks;              /* NULL: all 0                                                  */
  uint64_t num_keys;
  int32_t edge_type;                 /* positive type of `ON <edge>' (the binding resolved the name) */
  const uint8_t* const* yield_exprs; /* Expression::encode bytes per YIELD column                    */
  const uint32_t* yield_lens;
  int32_t num_yields;                /* 0: every column of the edge's latest schema, in schema order */
  int32_t distinct;                  /* YIELD DISTINCT                                               */
} nbg_fetch_edges_request;
int32_t nbg_fetch_edges(nbg_engine* e, const nbg_rows* in, const nbg_fetch_edges_request* req, nbg_rows** out);

/* ---- RowSetWriter bytes of a device-resident result (InterimResult's form) -----------------
 * What graphd makes of every result before the next executor, the client or a fallback path sees
 * it: an InterimResult, i.e. a schema plus the RowSetWriter bytes of every row
 * (GoExecutor.cpp:707-779, InterimResult.cpp:602-640).  nbg_rows_encode produces those bytes where
 * the rows lie and delivers them in pinned host memory, so the caller adds them with
 * RowSetWriter::addAll and builds the schema from nbg_rowset_col_type and its own column names;
 * no row passes through a RowWriter on the host.
 * Input: a device-resident result of the same single engine: a GO result (nbg_go_device,
 * nbg_go_execute with device = 1, nbg_go_wait, nbg_go_piped) or the output of any stage above.  It
 * stays valid and unchanged.  The call runs under the engine lock on the engine's stream; its
 * scratch and the device copy of the bytes are released before it returns.  The result does not
 * depend on `in` after the call; it must be freed (nbg_rowset_free) before nbg_destroy.
 * The bytes (byte-exact): the concatenation, in `in`'s fetch order (segment order, the order
 * nbg_rows_fetch delivers), of varint(len(row)) + row for every row (RowSetWriter.cpp:21-33), with
 * row = RowWriter(schema) << cell_0 << ...; encode() under schema version 0 (RowWriter.cpp:26-95,
 * RowWriter.inl:9-45):
 *   header   one byte, offsetBytes - 1, with offsetBytes = calcOccupiedBytes(cord size): 1 below 256
 *            bytes of cord, 2 below 65,536, 3 above; set whether or not the row has offsets;
 *   offsets  the cord's size after column 16 and after column 32 (RowWriter.h:143-148), each
 *            offsetBytes wide, little endian: 0, 1 or 2 of them (NBG_MAX_YIELDS is 32);
 *   cord     the cells by nbg_rows_col_type: INT / TIMESTAMP folly::encodeVarint of the payload as
 *            uint64_t (a negative value takes 10 bytes); VID 8 bytes, little endian; DOUBLE the 8
 *            payload bytes; BOOL one byte, 0 or 1; STRING varint(length), then the bytes — the
 *            dictionary's for a dictionary code, else the constant outside the dictionary that the
 *            cell's OVER type spells in that column.
 * The stored value of an aligned result is what InterimResult::getRows took back from the written
 * row (go.cpp prepare_schema), so encoding the stored cell by the column's type reproduces what
 * RowWriter wrote: a BOOL written into an INT column was one zero byte, is stored as INT 0 and is
 * written as varint 0, the same byte.
 * Statuses, in this order:
 *  1. NBG_E_INVALID_ARGUMENT: a null argument; `in` of another engine or host-only.
 *  2. NBG_E_UNSUPPORTED: a partitioned engine (each rank's rows could be encoded rank-locally and
 *     joined with RowSetWriter::addAll; not built).
 *  3. `in` has no rows: NBG_OK, a rowset of len 0 and rows 0 (nbg_rowset_data is NULL) that still
 *     reports the columns' types.
 *  4. Device scope: see "Device limits" (NBG_E_UNSUPPORTED; the caller then fetches `in` and runs
 *     its RowWriter loop).
 *  5. NBG_E_OUT_OF_MEMORY: a device or pinned allocation failed.
 * Three launches (DESIGN.md "RowSet encoding of device rows"): the rows' lengths, an exclusive scan
 * of the per-chunk byte sums (one 8-byte readback sizes the output), and the encoding through an
 * LDS staging buffer that is streamed out 16 bytes per lane. */
typedef struct nbg_rowset nbg_rowset;
int32_t nbg_rows_encode(nbg_engine* e, const nbg_rows* in, nbg_rowset** out);
const uint8_t* nbg_rowset_data(const nbg_rowset* rs);       /* pinned host memory, RowSetWriter::data() */
uint64_t nbg_rowset_len(const nbg_rowset* rs);
int64_t  nbg_rowset_rows(const nbg_rowset* rs);
int32_t  nbg_rowset_num_cols(const nbg_rowset* rs);
int32_t  nbg_rowset_col_type(const nbg_rowset* rs, int32_t col);   /* NBG_T_*: the SchemaWriter's field type; -1 out of range */
void     nbg_rowset_free(nbg_rowset* rs);
/* NBG_T_* of a result column (Collector::getSchema's type, what the row's writer and reader go by):
 * the result schema's entry, or the kind's natural type where it names none (INT, DOUBLE, BOOL,
 * STRING; the rule of nbg_set_op's checkSchema above); -1 out of range. */
int32_t  nbg_rows_col_type(const nbg_rows* r, int32_t col);

/* ---- Device-resident rows from RowSetWriter bytes (the inverse of nbg_rows_encode) ----------
 * The way back in.  When a stage answers NBG_E_UNSUPPORTED the reference's own executor produces
 * an InterimResult on the host, and so does every `$var` a CPU executor assigned: a schema plus
 * RowSetWriter bytes.  nbg_rows_decode makes an ordinary device-resident nbg_rows of them, the
 * device form of what InterimResult::getRows / buildIndex do with a RowReader per row
 * (InterimResult.cpp:74-140, 158-250; RowReader.cpp:213-258; RowSetReader.cpp), so the clauses
 * after the fallback run on the device again.
 * The caller keeps `data`; the result does not depend on it after the call.  The call runs under
 * the engine lock on the engine's stream; the pinned block and the device copy of the bytes are
 * released before it returns.
 * The result: a device-resident nbg_rows in a workspace of its own — one segment in the input's
 * row order, one OVER position, no string constants outside the dictionary, no derived strings,
 * neither misaligned nor FLOAT, no step statistics, nbg_rows_edges_scanned = 0.  Every nbg_rows_*
 * accessor works on it and every stage above takes it, nbg_go_piped and nbg_rows_encode included.
 * nbg_rows_col_type reports col_types; nbg_rows_col_kind follows the type: INT / VID / TIMESTAMP
 * NBG_V_INT, DOUBLE NBG_V_DOUBLE, BOOL NBG_V_BOOL, STRING NBG_V_STRING.
 * The bytes (the read side of what nbg_rows_encode documents): row after row, varint(len(row))
 * and the row.  The row's header byte holds offsetBytes - 1 in its low 3 bits and the count of
 * schema-version bytes in its top 3; the version bytes are skipped, then num_cols >> 4 block
 * offsets of offsetBytes each (the cord is walked in order, so they are not needed), then the
 * cord's cells are read by type:
 *   INT / TIMESTAMP  a varint of at most 10 bytes, read as uint64_t, stored as int64_t;
 *   VID, DOUBLE      8 bytes, little endian;
 *   BOOL             one byte, stored as 0 / 1 (a byte other than 0 / 1 is unspecified);
 *   STRING           varint(length) and the bytes; the stored cell is the dictionary code of those
 *                    bytes (2 x the index in the sorted dictionary), and the empty string takes the
 *                    code every other route gives it whether or not the dictionary holds it.
 * Bytes of the cord left over after the last cell are ignored, as RowReader ignores them.
 * Statuses, in this order:
 *  1. NBG_E_INVALID_ARGUMENT: a null argument; num_cols < 1; a col_types entry outside
 *     NBG_T_BOOL..NBG_T_TIMESTAMP; len > 0 with null data.  (Then NBG_E_STATE before nbg_finalize.)
 *  2. NBG_E_UNSUPPORTED: a partitioned engine.
 *  3. len == 0: NBG_OK, a result of no rows with num_cols columns of those types and kinds.
 *  4. Device scope: see "Device limits" (NBG_E_UNSUPPORTED; the caller keeps the host route): a
 *     FLOAT field, more than NBG_MAX_YIELDS fields, 2^32 rows or more, a chunk of 2,048 rows whose
 *     bytes reach 4 GiB.
 *  5. NBG_E_INVALID_ARGUMENT, malformed bytes the host walk finds before any launch: a length
 *     prefix over 10 bytes or running past len; a row running past len; a row of length 0 (it has
 *     no header byte); a row shorter than its own header.  The message names the row and the byte.
 *  6. NBG_E_INVALID_ARGUMENT, found on the device: a cell that would read past its row's end (a
 *     varint cell over 10 bytes included).  The message counts such rows and names the first row
 *     and column.
 *  7. NBG_E_UNSUPPORTED: a STRING cell whose bytes are not in the snapshot's dictionary;
 *     nbg_last_error says how many.
 *  8. NBG_E_OUT_OF_MEMORY: a device or pinned allocation failed.
 * Row starts are found by a host walk of the length-prefix chain (it is sequential, and it is the
 * validating path); the bytes, one 8-byte start per chunk of 2,048 rows and a 32-bit offset per
 * row go up in one DMA from a pinned block, and one launch reads the cells, a lane per row
 * (DESIGN.md "RowSet decoding into device rows").  No input can make the kernel read outside the
 * uploaded bytes: every read is bounded by the row's end, and the row's end by len. */
typedef struct {
  const uint8_t* data;        /* RowSetWriter::data(): varint(len(row)) + row, row after row */
  uint64_t len;
  const int32_t* col_types;   /* NBG_T_* per schema field, in field order */
  int32_t num_cols;
} nbg_rowset_view;
int32_t nbg_rows_decode(nbg_engine* e, const nbg_rowset_view* rs, nbg_rows** out);

/* ---- FIND SHORTEST | ALL PATH (FindPathExecutor semantics) ----------------------------- */
typedef struct {
  const int64_t* from;           /* de-duplicated by the callee (VerticesClause::prepare)    */
  uint64_t num_from;
  const int32_t* edge_types;
  int32_t num_edge_types;
  int32_t over_all;
  const int64_t* to;
  uint64_t num_to;
  uint32_t upto;                  /* UPTO N STEPS, default 5 (parser.yy:858-861)              */
  int32_t shortest;               /* 1 = SHORTEST, 0 = ALL                                     */
} nbg_path_request;

/* Each path is an entry list [v0, t0, r0, v1, t1, r1, ..., vk] (vertex, edge type, ranking …)
 * — the graph.thrift Path entry_list (graph.thrift:58-73) with edge names as types.
 * SHORTEST returns at most one path per target: the minimum hop count, ties broken by the
 * lexicographically smallest entry list (the reference's tie-break is iteration order). */
int32_t nbg_find_path(nbg_engine* e, const nbg_path_request* req, nbg_paths** out);
/* Asynchronous FIND PATH: up to NBG_QUERY_SLOTS (default 6) one-pair SHORTEST queries of a
 * single (non-partitioned) engine in flight, each on its own device workspace and HIP stream;
 * every other request runs inside nbg_find_path_submit.  When every slot is busy the oldest query
 * is completed first (its result stays in its ticket).  nbg_find_path_wait returns the result with
 * nbg_find_path's semantics (and status) and frees the ticket; tickets must be waited for before
 * nbg_destroy (outstanding ones are reclaimed there). */
typedef struct nbg_path_ticket nbg_path_ticket;
int32_t nbg_find_path_submit(nbg_engine* e, const nbg_path_request* req, nbg_path_ticket** out);
int32_t nbg_find_path_wait(nbg_path_ticket* ticket, nbg_paths** out);

/* n independent FIND PATH requests at once (a graphd serving many FindPathExecutor queries,
 * src/graph/FindPathExecutor.cpp:145-411, each with its own result): out[i] / rcs[i] receive
 * request i's paths (free each with nbg_paths_free; NULL when rcs[i] != NBG_OK) and status.
 * One-pair SHORTEST requests on a single engine (UPTO <= 32) run as rolling device runs over
 * NBG_SP_BATCH (default 64, at most 64) contexts: every launch serves every context, and a
 * context takes the next queued pair as soon as its pair is done (UPTO over 32: fixed batches of
 * at most 32).  Each context holds a 16-byte label record per vertex and 5 lists of a quarter of
 * the vertices (NBG_SP_BATCH_LIST; ~1.2 GB at RMAT-26; a pair outgrowing them runs again on the
 * engine's full-size context, nbg_stats.path_batch_reruns); as many are made as HBM allows.  Other
 * requests run as nbg_find_path would.  Results equal nbg_find_path's.  Every request gets its
 * status in rcs[i] (out[i] is NULL exactly when rcs[i] != NBG_OK), also when the batch itself
 * fails part way (the requests that did not run carry that failure's code).  Returns NBG_OK
 * unless the batch itself could not run (arguments, device set-up). */
int32_t nbg_find_path_batch(nbg_engine* e, const nbg_path_request* reqs, uint64_t n, nbg_paths** out,
                            int32_t* rcs);
/* Allocate the one-pair SHORTEST contexts now instead of at their first query (what a server
 * does at start-up): the engine's own, `slots` of nbg_find_path_submit's (at most NBG_QUERY_SLOTS)
 * and `batch` of nbg_find_path_batch's (at most NBG_SP_BATCH; as many as fit in HBM, at least
 * one, else NBG_E_OUT_OF_MEMORY).  A one-pair context holds ~76 B per vertex plus its lists' tile
 * splits, a batch context ~31 B.  No-op on a partitioned engine. */
int32_t nbg_path_reserve(nbg_engine* e, int32_t slots, int32_t batch);
int64_t nbg_paths_count(const nbg_paths* p);
int64_t nbg_path_len(const nbg_paths* p, int64_t i);
const int64_t* nbg_path_entries(const nbg_paths* p, int64_t i);
/* Adjacency entries the search scanned (both directions; TEPS numerator). */
uint64_t nbg_paths_edges_scanned(const nbg_paths* p);
/* Diagnostic: launch batches the device level loop needed for this result (1: the first chain
 * finished it; more: the host continued it; 0: the host-driven loop answered). */
uint32_t nbg_paths_chain_batches(const nbg_paths* p);
void nbg_paths_free(nbg_paths* p);

/* ---- GetNeighbors (storage boundary: StorageServiceHandler::future_getBound) -------------
 * Columnar mirror of GetNeighborsRequest / QueryResponse (src/interface/storage.thrift:47-106,
 * 153-161) served by QueryBoundProcessor (src/storage/QueryBoundProcessor.cpp:16-220,
 * QueryBaseProcessor.inl:60-562): per requested (part, vid), tag rows of the SOURCE columns and,
 * per requested edge type that has return columns, the RowSet of its edges in key order
 * (latest version, storage-side filter with keep-on-error, first max_edge_returned_per_vertex
 * accepted edges).  Rows are the exact RowWriter / RowSetWriter bytes storaged would send
 * (src/dataman/RowWriter.cpp:26-95, RowSetWriter.cpp:21-43), so a thrift adapter copies them
 * into QueryResponse unchanged.  Request-level errors (unknown schema / prop, an invalid filter)
 * are reported as one failed code per requested part, like QueryBaseProcessor.inl:529-535;
 * parts this engine does not serve fail with NBG_E_PART_NOT_FOUND.  The edge walk and filter
 * run on the device (one expansion over the requested vertices per edge type). */
#define NBG_PROP_SOURCE 1
#define NBG_PROP_DEST   2
#define NBG_PROP_EDGE   3
typedef struct {
  int32_t owner;                  /* NBG_PROP_SOURCE / _DEST (tag prop) or _EDGE               */
  int32_t id;                     /* tag id, or signed edge type                               */
  const char* name;               /* prop name; _src / _dst / _type / _rank for edge keys      */
} nbg_prop_def;

typedef struct {
  const int32_t* parts;           /* part of each vid: the map<PartitionID, list<VertexID>>   */
  const int64_t* vids;            /*   flattened (one entry per requested vid)                 */
  uint64_t num_vids;
  const int32_t* edge_types;      /* signed: negative = in-edges                               */
  int32_t num_edge_types;
  const uint8_t* filter;          /* Expression::encode bytes; NULL/0 = none                   */
  uint32_t filter_len;
  const nbg_prop_def* return_columns;
  int32_t num_return_columns;
} nbg_gn_request;

typedef struct nbg_gn_response nbg_gn_response;
int32_t nbg_get_neighbors(nbg_engine* e, const nbg_gn_request* req, nbg_gn_response** out);
/* result.failed_codes: (code, part) pairs; latency_in_us */
int32_t nbg_gn_num_failed(const nbg_gn_response* r);
int32_t nbg_gn_failed(const nbg_gn_response* r, int32_t i, int32_t* code, int32_t* part);
int32_t nbg_gn_latency_us(const nbg_gn_response* r);
/* vertex_schema (is_edge = 0) / edge_schema (is_edge = 1): entries, then columns of entry i */
int32_t nbg_gn_num_schemas(const nbg_gn_response* r, int32_t is_edge);
int32_t nbg_gn_schema(const nbg_gn_response* r, int32_t is_edge, int32_t i, int32_t* id, int32_t* ncols);
int32_t nbg_gn_schema_col(const nbg_gn_response* r, int32_t is_edge, int32_t i, int32_t c, const char** name,
                          int32_t* type);
/* vertices[i]: vid, tag_data[k] = (tag, row bytes), edge_data[k] = (type, RowSet bytes) */
int64_t nbg_gn_num_vertices(const nbg_gn_response* r);
int64_t nbg_gn_vertex_id(const nbg_gn_response* r, int64_t i);
int32_t nbg_gn_vertex_num_tags(const nbg_gn_response* r, int64_t i);
int32_t nbg_gn_vertex_tag(const nbg_gn_response* r, int64_t i, int32_t k, int32_t* tag, const uint8_t** data,
                          uint64_t* len);
int32_t nbg_gn_vertex_num_edges(const nbg_gn_response* r, int64_t i);
int32_t nbg_gn_vertex_edges(const nbg_gn_response* r, int64_t i, int32_t k, int32_t* type, const uint8_t** data,
                            uint64_t* len);
/* Adjacency entries the device walk returned (after the filter and cap). */
uint64_t nbg_gn_edges(const nbg_gn_response* r);
void nbg_gn_free(nbg_gn_response* r);

/* ---- boundStats (StorageServiceHandler::future_boundStats -> QueryStatsProcessor) ---------
 * The GetNeighbors request with a StatType per return column (storage.thrift PropDef.stat):
 * one row of SUM / COUNT / AVG over the collected values (QueryStatsProcessor.cpp:16-130,
 * StatsCollector in Collector.h:76-109): tag props of the requested vertices, edge props of the
 * accepted edges; _src/_dst are not collected, bool/string only count; SUM/AVG need a numeric
 * column (else NBG_E_IMPROPER_DATA_TYPE per part).  `data` is the encoded row. */
#define NBG_STAT_SUM   1
#define NBG_STAT_COUNT 2
#define NBG_STAT_AVG   3
typedef struct nbg_stats_response nbg_stats_response;
int32_t nbg_bound_stats(nbg_engine* e, const nbg_gn_request* req, const int32_t* stats, nbg_stats_response** out);
int32_t nbg_stats_num_failed(const nbg_stats_response* r);
int32_t nbg_stats_failed(const nbg_stats_response* r, int32_t i, int32_t* code, int32_t* part);
int32_t nbg_stats_num_cols(const nbg_stats_response* r);
/* column c: name, NBG_T_INT / NBG_T_DOUBLE, value (int64 or double bits) */
int32_t nbg_stats_col(const nbg_stats_response* r, int32_t c, const char** name, int32_t* type, int64_t* bits);
int32_t nbg_stats_data(const nbg_stats_response* r, const uint8_t** data, uint64_t* len);
void nbg_stats_free(nbg_stats_response* r);

/* ---- in-library kernel timing (HIP events on the engine's stream) ----------------------- */
typedef struct {
  const char* name;           /* kernel name (static string)                                  */
  uint64_t launches;
  double total_ms;            /* sum of event-measured launch durations                        */
  double algo_bytes;          /* algorithmic HBM bytes of those launches */
} nbg_kernel_stat;
/* enable = 1 starts (and resets) timing of every launch; 2 times only the final-step /
 * shortest-path expansion kernels (two events per query: minimal perturbation of the timed
 * region); 0 stops timing.  Mode 1 also times nbg_order_by's launches: k_ob_iota, k_ob_hist,
 * k_ob_pick, k_ob_compact (the first-K selection), k_ob_image, ob_radix_sort, k_ob_gather,
 * k_ob_copy (DESIGN.md "ORDER BY / LIMIT"), and nbg_set_op's: k_so_insert, k_so_probe, k_so_emit,
 * k_so_copy (DESIGN.md "Set operations over device rows"), and nbg_yield's: k_yr_filter,
 * k_yr_scan, k_yr_emit (DESIGN.md "YIELD over device rows"), and nbg_fetch_vertices':
 * k_fv_resolve, k_fv_emit (DESIGN.md "FETCH PROP over device rows"), and nbg_fetch_edges':
 * k_fe_resolve, k_fe_emit (DESIGN.md "FETCH PROP ON <edge> over device rows"). */
/* ... and nbg_yield_agg's: k_ya_reduce, k_ya_finish (DESIGN.md "Aggregate YIELD over device rows");
 * its COUNT_DISTINCT columns are counted under nbg_yield's and nbg_set_op's kernels. */
/* ... and nbg_go_piped's: k_gp_resolve, k_gp_table, k_gp_degrees, k_gp_emit, k_gp_compact (DESIGN.md
 * "GO over device rows"); the hops after them are counted under nbg_go's kernels. */
/* ... and nbg_rows_encode's: k_re_size, k_re_scan, k_re_emit (DESIGN.md "RowSet encoding of device
 * rows"); k_re_emit's algorithmic bytes are the cells and row lengths read plus the bytes written. */
/* ... and nbg_rows_decode's: k_rd_cells (DESIGN.md "RowSet decoding into device rows"); its algorithmic
 * bytes are the row bytes and offsets read plus 8 x the cells written.  Two entries in front of it,
 * rd_host_walk and rd_host_upload, are host-clock times of the call's host parts: the walk of the
 * length prefixes, and the copy into the pinned block plus the DMA (which the call waits for only
 * while the profile is on). */
/* ---- FIND PATH replica of a partitioned engine (replica.hip) ---------------------------------
 * A partitioned engine (num_gpus > 1) also builds, at nbg_finalize (collectively), a replica of
 * every rank's path CSRs (offsets, neighbour ids and vids, ranks; no property columns) when it fits
 * in free HBM.  While it is in use, nbg_find_path / _submit / _batch / nbg_path_reserve run on it
 * RANK-LOCALLY: no collective, each rank may answer different requests, and the results equal the
 * single engine's over the same records.  Without it they are collectives over the partitioned
 * snapshot (every rank calls them with the same requests).
 * nbg_set_path_replica: before nbg_finalize, whether to build it (default: NBG_PATH_REPLICA, 1);
 * after, whether FIND PATH uses it (1 needs a built replica: else NBG_E_STATE).  It replaces
 * no reference interface (graphd reaches storaged for every FindPathExecutor round). */
int32_t nbg_set_path_replica(nbg_engine* e, int32_t mode);
int32_t nbg_path_replica_active(const nbg_engine* e);   /* 1: FIND PATH runs on the replica */

int32_t nbg_profile(nbg_engine* e, int32_t enable);
/* Copies up to cap kernel records; returns the number of kernels. */
int32_t nbg_profile_read(const nbg_engine* e, nbg_kernel_stat* out, int32_t cap);

/* ---- multi-GPU: partitioned engine ------------------------------------
 * With nbg_config.num_gpus = G > 1 an engine holds only the parts p with p % G == rank
 * (CreateSpaceProcessor.cpp:84-95, GPUs as storaged hosts) and every query is a collective:
 * all G engines must run the same nbg_go calls (same arguments, in the same order), the way
 * StorageClient::getNeighbors fans one request out to every host (StorageClient.cpp:94-124).
 * Per GO hop each rank expands its local frontier, and the per-step dst SET
 * (GoExecutor::getDstIdsFromResp, GoExecutor.cpp:501-541) is formed by one bitmap all-to-all:
 * rank q receives the candidates it owns.  Final-step rows stay on the rank that produced
 * them (the result is the union over ranks); nbg_rows_step_stats / nbg_rows_edges_scanned
 * report the whole query (summed over ranks).  The communicator must be attached before
 * nbg_finalize (the loader exchanges vertex dictionaries to build global neighbour ids).
 * nbg_find_path is collective too: each BFS level exchanges its candidate bitmap and the owner
 * claims (meet / target tests local at the owner, FindPathExecutor.cpp:218-290), sizes are summed
 * over ranks, and every rank returns the same paths. */
#define NBG_UNIQUE_ID_BYTES 128
/* RCCL unique id (ncclGetUniqueId); rank 0 creates it and ships it to the others. */
int32_t nbg_comm_unique_id(uint8_t out[NBG_UNIQUE_ID_BYTES]);
/* One process per GPU: RCCL communicator over xGMI (ncclCommInitRank); collective per rank. */
int32_t nbg_comm_init(nbg_engine* e, const uint8_t id[NBG_UNIQUE_ID_BYTES], int32_t world, int32_t rank);
/* Several engines of ONE process (engine i has rank i, num_gpus == n): an in-process group whose
 * collectives copy between the engines' buffers.  Each engine is then driven by its own host
 * thread (finalize and every query), exactly as the RCCL ranks are. */
int32_t nbg_comm_init_local(nbg_engine* const* engines, int32_t n);
/* Failure semantics of a partitioned engine.  The reference keeps a query alive when some
 * storaged parts fail and reports them (StorageClient.inl:112-136, GoExecutor.cpp:424-442); a
 * collective engine cannot run a hop without one of its ranks, so a query fails on EVERY rank
 * with the same code instead:
 *   - a rank-local failure before the query's first collective (allocation, a start list whose
 *     edges exceed one rank's list limit, ...) reaches every rank: every rank returns the code of
 *     the lowest-ranked rank that failed, and the engines stay usable.  For GO without $- / $var
 *     inputs (YIELD DISTINCT included) the failing rank still takes part in the query's
 *     collectives and its status travels with the query's statistics (no extra round trip):
 *     nbg_go_execute fails on every rank; nbg_go_submit returns a ticket on every rank (so every
 *     rank's query slots stay in step) and nbg_go_wait on it returns the code.  Other statements (and
 *     FIND PATH) agree in one small all-reduce before the query, so every rank's call fails;
 *   - a failure between collectives (a device error on one rank) aborts the communicator; the
 *     peers' pending collectives fail (in-process group at once, RCCL when their bounded wait of
 *     NBG_COMM_TIMEOUT_S seconds, default 120, expires) and every later collective call fails
 *     with NBG_E_DEVICE.
 * nbg_comm_abort aborts the engine's communicator(s) from any thread (ncclCommAbort for RCCL):
 * a host watchdog uses it to release a rank blocked in a collective.  Not under the engine
 * lock.  nbg_comm_aborted: 1 after an abort (the engine must be rebuilt), else 0. */
int32_t nbg_comm_abort(nbg_engine* e);
int32_t nbg_comm_aborted(const nbg_engine* e);
/* Testing hook: the next `count` queries of this engine fail at `site` exactly as a real failure
 * there would (the failure paths above are otherwise hard to reach on purpose). */
#define NBG_FAULT_ALLOC  1   /* the query's workspace / held-result hand-over allocation fails */
#define NBG_FAULT_DEVICE 2   /* partitioned GO: a device error after the query's first collective */
#define NBG_FAULT_STREAM 3   /* nbg_go_submit: the query slot's stream cannot be created */
int32_t nbg_inject_fault(nbg_engine* e, int32_t site, int32_t count);
/* The edge records this engine staged for signed edge type `type` (+t: out-edges keyed at src,
 * -t: in-edges keyed at dst), in load order, before nbg_finalize: a partitioned rank keeps the
 * records of the parts it serves (CreateSpaceProcessor.cpp:84-95 with GPUs as hosts), so the
 * ranks' lists partition the load.  Host only (no device call).  *n = the record count; up to
 * `cap` of them are written to src / dst / rank (any may be NULL).  NBG_E_STATE once finalized. */
int32_t nbg_staged_edges(const nbg_engine* e, int32_t type, int64_t* src, int64_t* dst, int64_t* rank, uint64_t cap,
                         uint64_t* n);

#ifdef __cplusplus
}
#endif
#endif /* NEBULA_AMD_NBG_H_ */
