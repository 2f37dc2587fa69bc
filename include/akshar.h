/*
 * akshar.h — C-ABI of the MI355X batch tokenization engine (libakshar: akshar_amd/_akshar_hip.so).
 *
 * The reference (Bhasha-Open/Akshar, pure Python) has no FFI: its boundary is the Python API
 * (src/akshar/tokenizer.py:18-288, src/akshar/__init__.py:12-109) plus a duck-typed engine seam
 * `self.model.encode(str).ids` / `self.model.EncodeAsIds(str)` (tokenizer.py:153-156,190-193).
 * Each entry point below replaces one reference interface, batched: rows are packed UTF-8 in one
 * byte buffer with u64 row offsets, every output is a packed buffer plus u64 row offsets.
 *
 * Conventions
 *  - Every call returns an int status (AK_OK or a negative AK_ERR_*); ak_last_error() returns a
 *    thread-local message for the last failure on the calling thread.
 *  - All array arguments of the batch calls are DEVICE pointers (hipMalloc / torch CUDA tensors)
 *    on the current HIP device; `stream` is a hipStream_t (NULL = default stream). Batch calls
 *    only enqueue work: results are valid after the stream is synchronized.
 *  - Input: `in` holds offs[n] bytes (offs[0] == 0, offs non-decreasing). Each row is one string
 *    of the reference API. The buffer must stay readable through offs[n] rounded up to 16 bytes (rows are
 *    read in aligned 16-byte blocks). `in` needs no alignment: it may point anywhere into a larger
 *    allocation (a sub-range of another batch), and what precedes it is never taken for row text. The
 *    bytes after offs[n] may hold anything: they are loaded with the last block but never decoded,
 *    so the last row ends at offs[n] whatever follows it (a combining mark, a UTF-8 lead byte, ...).
 *    The same holds for the ids of the decode calls.
 *  - Output sizing: callers pass a capacity `cap` (elements). out_offs[0..n] is always written;
 *    the total is out_offs[n]. If out_offs[n] > cap, the call still returns AK_OK but the output
 *    elements are incomplete: re-run with cap >= out_offs[n] (the bound helpers below give caps
 *    that are always sufficient). Nothing is stored at or past element `cap` of an output array
 *    (cap == out_offs[n] exactly is enough, cap == 0 is allowed), past out_offs[n] or past
 *    row_status[n - 1]; out_offs and row_status are complete at any capacity. A short capacity is
 *    the caller's matter, not an engine overflow: ak_ws_check() still returns AK_OK after such a
 *    call, and the workspace keeps no state from it (the re-run may use the same workspace).
 *  - row_status (optional, u8[n], may be NULL): bit 0 = row had invalid UTF-8 (decoded as U+FFFD
 *    per byte). Bit 2 (AK_ROW_LIMIT) is only ever set together with an engine-bug error from
 *    ak_ws_check(): no row length is rejected (see "Row lengths").
 *  - Row lengths: there is no per-row limit. Rows run in up to three tiers: the fast kernels
 *    (small private buffers), the slow tier (per-thread pool regions of AK_SLOW_TIER_ENTRIES code
 *    points per NFC segment / symbols per BPE pre-token or SentencePiece word), and the huge tier,
 *    whose pool is sized from the longest row past the slow tier (one extra host read-back; about
 *    300 bytes of device memory per input byte of that row). A call whose huge tier cannot be
 *    allocated fails with AK_ERR_NOMEM; it never returns a short or empty row.
 *  - Models and workspaces are not thread-safe for concurrent calls on different streams with the
 *    same workspace; models are immutable after creation and may be shared.
 */
#ifndef AKSHAR_H
#define AKSHAR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AK_OK 0
#define AK_ERR_ARG (-1)
#define AK_ERR_HIP (-2)
#define AK_ERR_UNSUPPORTED (-3)
#define AK_ERR_NOMEM (-4)

/* normalize_text flags (normalize.py:117 `normalize_text(text, normalize_roman, clean_hinglish)`) */
#define AK_NORM_LOWER 1 /* normalize_roman=True: 'LATIN' in name(c) -> c.lower()  (normalize.py:21-45) */
#define AK_NORM_CLEAN 2 /* clean_hinglish=True: allowlist filter + elongation collapse (:92-114) */
#define AK_NORM_DEFAULT (AK_NORM_LOWER | AK_NORM_CLEAN)
#define AK_RAW (-1)     /* segment/switches on the raw row (the free functions on unnormalized text) */

/* ak_normalize only: AK_NORM_STAGES | any AK_ST_* runs exactly the selected steps of normalize_text,
 * in its order, each of which the reference also exports on its own (normalize.py:13-114):
 *   normalize_unicode  AK_ST_NFC          semantic_normalize AK_ST_LOWER
 *   filter_garbage     AK_ST_FILTER       remove_elongations AK_ST_ELONG
 *   normalize_hinglish AK_ST_FILTER | AK_ST_ELONG   (:110-114; no NFC, no lowercasing)
 * AK_NORM_STAGES | AK_ST_NFC | AK_ST_LOWER | AK_ST_FILTER | AK_ST_ELONG == AK_NORM_DEFAULT. */
#define AK_NORM_STAGES 16
#define AK_ST_NFC 1    /* unicodedata.normalize('NFC') (:13-18) */
#define AK_ST_LOWER 2  /* 'LATIN' in name(c) -> c.lower() (:21-45) */
#define AK_ST_FILTER 4 /* allowlist filter (:92-107) */
#define AK_ST_ELONG 8  /* re.sub(r'(.)\1{2,}', r'\1') (:48-56) */

/* per-row status bits */
#define AK_ROW_BAD_UTF8 1u
#define AK_ROW_LIMIT 4u

/* per-thread capacity of the slow tier (code points of one NFC segment, symbols of one BPE
 * pre-token, chars of one SentencePiece word); longer ones run in the huge tier */
#define AK_SLOW_TIER_ENTRIES 4096

typedef struct ak_bpe ak_bpe; /* device-resident BPE model (HF tokenizers models.BPE) */
typedef struct ak_spm ak_spm; /* device-resident SentencePiece unigram model */
typedef struct ak_ws ak_ws;   /* device scratch, grows on demand; one per stream */

const char *ak_last_error(void);
int ak_version(void);
/* Device self-test of the wave64 primitives the tile kernels rely on (DPP prefix scan, readlane
 * broadcast, ballot): AK_OK, or AK_ERR_HIP with the first mismatch in ak_last_error(). */
int ak_selftest(void);

int ak_ws_create(ak_ws **out);
void ak_ws_free(ak_ws *ws);
/* Kernel choice for this workspace's calls with the normalize_text defaults (flags 3: BPE and
 * SentencePiece encodes, normalize, segment / switches of normalized rows, analyze): path 1 =
 * tile-cooperative single pass (default; a wave packs up to tile_rows rows, 1..16, default 16,
 * into each tile, as many as fit its byte buffer), 0 = one lane per row (the staged row kernels). */
int ak_ws_set_tiling(ak_ws *ws, int bpe_path, int tile_rows);
/* Synchronous health check after a batch: AK_ERR_HIP if the last call flagged an internal
 * overflow (a row producing more output than its staging slot bound, or overflowing the huge
 * tier; never observed). A call whose `cap` was short of out_offs[n] flags nothing: AK_OK. */
int ak_ws_check(ak_ws *ws);

/* Replaces Tokenizer.from_file(path) (tokenizer.py:96-97) for the model cli.py:276-299 trains:
 * NFKC -> Whitespace -> BPE(unk_token=None) -> "<s> $A </s>".
 * single_cp/single_id: the single-code-point vocab entries; merges: n_merges x {left, right, new}
 * in rank order (rank = row index); bos/eos: the template's special ids. Host pointers. */
int ak_bpe_create(uint32_t n_single, const uint32_t *single_cp, const uint32_t *single_id,
                  uint32_t n_merges, const uint32_t *merges, uint32_t bos, uint32_t eos, ak_bpe **out);
void ak_bpe_free(ak_bpe *m);
/* The tile path's pre-token result cache, built by ak_bpe_create (HF BPE's per-word cache,
 * tokenizer.py:96-97,193, made exact at load: keys are the char-id sequences of merged tokens whose
 * merge_all is that one id). info[0] table slots (0 = no cache: not a tile-path model, or AK_PTC=0
 * in the environment), [1] keys found, [2] keys stored, [3] merged-token sequences whose merge_all is
 * not one id (never stored). */
int ak_bpe_cache_info(const ak_bpe *m, uint64_t info[4]);
/* The tokenizer's added tokens (tokenizer.json "added_tokens": <pad> <unk> <s> </s> <mask> for
 * cli.py:283-285), all normalized=false / lstrip=rstrip=single_word=false: HF's AddedVocabulary
 * splits the text it receives on them (leftmost-longest) BEFORE the NFKC normalizer, each match
 * becoming its id and each piece between encoded on its own. Only reachable with
 * clean_hinglish=False (the allowlist drops '<' '>' '/'); a token made only of allowlisted chars is
 * AK_ERR_UNSUPPORTED. n tokens <= AK_MAX_ADDED, each 1..16 code points: cps packed with
 * cp_offs[n+1]. Host pointers; replaces any previous set. */
#define AK_MAX_ADDED 64
int ak_bpe_set_added(ak_bpe *m, uint32_t n, const uint32_t *cps, const uint32_t *cp_offs, const uint32_t *ids);

/* Replaces SentencePieceProcessor.Load(path) (tokenizer.py:88-90) for the unigram model
 * cli.py:232-248 trains (identity normalizer, byte_fallback). pieces: n UTF-8 strings packed in
 * piece_bytes with piece_offs[n+1]; scores float[n]; types u8[n] (sentencepiece_model.proto
 * enum: 1 NORMAL 2 UNKNOWN 3 CONTROL 4 USER_DEFINED 5 UNUSED 6 BYTE); byte_ids[256]: ids of
 * <0x00>..<0xFF>. Host pointers. */
int ak_spm_create(uint32_t n, const uint8_t *piece_bytes, const uint64_t *piece_offs, const float *scores,
                  const uint8_t *types, int32_t unk_id, const int32_t *byte_ids, ak_spm **out);
void ak_spm_free(ak_spm *m);
/* The tile path's word cache, built by ak_spm_create when AK_SWC=1 is in the environment (off by
 * default: measured slower): the base-0 lattice solution (pieces and the smallest
 * winning margin) of every "▁"-initial piece string, solved at load; a hit is accepted under the
 * same rounding-bound test as a solved word. info[0] table slots (0 = no cache), [1] words found,
 * [2] words stored, [3] words whose solution holds an unknown char or more than 6 pieces (never
 * stored). */
int ak_spm_cache_info(const ak_spm *m, uint64_t info[4]);

/* Model files read inside the library (host code, no GPU needed to parse): a caller over the
 * C-ABI needs no tokenizer.json / protobuf parser of its own. Same acceptance rules as
 * ak_bpe_create / ak_spm_create above (and akshar_amd/models.py).
 * ak_bpe_load: HF tokenizer.json -> ak_bpe_create + ak_bpe_set_added + ak_bpe_set_vocab
 *   (replaces Tokenizer.from_file, tokenizer.py:96-97).
 * ak_spm_load: SentencePiece .model (ModelProto wire format) -> ak_spm_create
 *   (replaces SentencePieceProcessor.Load, tokenizer.py:88-90).
 * ak_model_load: model_type "bpe" (-> ak_bpe*) or "sentencepiece" (-> ak_spm*), the reference's
 *   aksharTokenizer(model_path, model_type) choice (tokenizer.py:54-102); ak_model_free likewise.
 *   The library keeps a set of its live handles: ak_model_free of a pointer that is not one (never
 *   created, or already freed) sets AK_ERR_ARG's message and touches nothing.
 * ak_model_info (parse only, no device): info[0] vocab / piece count, BPE: [1] single-char
 *   entries, [2] merges, [3] bos, [4] eos, [5] added tokens; SPM: [1] unk id; [7] a 64-bit FNV-1a
 *   of every array the loader would pass to the create calls, in their argument order. */
int ak_bpe_load(const char *path, ak_bpe **out);
int ak_spm_load(const char *path, ak_spm **out);
int ak_model_load(const char *path, const char *model_type, void **out);
void ak_model_free(void *h, const char *model_type);
int ak_model_info(const char *path, const char *model_type, uint64_t info[8]);

/* normalize_text(text, normalize_roman, clean_hinglish) (normalize.py:117-148) per row, flags
 * 0..3; or AK_NORM_STAGES | AK_ST_* for any subset of its steps (above).
 * out: UTF-8 bytes; a sufficient cap is ak_normalize_cap(). */
int ak_normalize(ak_ws *ws, int flags, const uint8_t *in, const uint64_t *offs, uint64_t n, uint8_t *out,
                 uint64_t cap, uint64_t *out_offs, uint8_t *row_status, void *stream);

/* segment_akshars(text, matras) (segment.py:40-125) per row: cluster END indices (code points,
 * relative to the row) of the normalized row (flags >= 0, as tokenize() without a model,
 * tokenizer.py:144-151) or of the raw row (flags == AK_RAW). */
int ak_segment(ak_ws *ws, int flags, int matras, const uint8_t *in, const uint64_t *offs, uint64_t n,
               uint32_t *ends, uint64_t cap, uint64_t *out_offs, uint8_t *row_status, void *stream);

/* detect_code_switches(text) (segment.py:150-201) per row: run END indices (code points) and
 * labels (0 other, 1 devanagari, 2 roman, 255 None = all-neutral row). */
int ak_switches(ak_ws *ws, int flags, const uint8_t *in, const uint64_t *offs, uint64_t n, uint32_t *ends,
                uint8_t *labels, uint64_t cap, uint64_t *out_offs, uint8_t *row_status, void *stream);

/* The front half of aksharTokenizer.explain(text) / tokenize(text, return_metadata=True)
 * (tokenizer.py:248-276, :146-147; segment.py:210-236), fused into ONE pass per row:
 * norm = normalize_text(text, flags) as UTF-8 (like ak_normalize), and on that normalized text
 * segment_akshars(norm, matras) cluster ENDs (like ak_segment with AK_RAW on norm) and
 * detect_code_switches(norm) run ENDs + labels (like ak_switches with AK_RAW on norm).
 * Three outputs, each with its own capacity and u64[n+1] offsets ([n] = required total). */
int ak_analyze(ak_ws *ws, int flags, int matras, const uint8_t *in, const uint64_t *offs, uint64_t n,
               uint8_t *norm, uint64_t norm_cap, uint64_t *norm_offs, uint32_t *clusters, uint64_t cl_cap,
               uint64_t *cl_offs, uint32_t *runs, uint8_t *labels, uint64_t run_cap, uint64_t *run_offs,
               uint8_t *row_status, void *stream);

/* aksharTokenizer(model, "bpe").encode(text) (tokenizer.py:167-193): normalize_text(flags) then
 * the HF pipeline; ids include <s> ... </s>. Any flags 0..3: with AK_NORM_CLEAN the normalized
 * text is over the allowlist (tile path for flags 3); without it (clean_hinglish=False) any text
 * reaches the tokenizer: added-token split, HF's full NFKC (Unicode 9 tables of tokenizers
 * 0.22.2) and the Whitespace pre-tokenizer over every code point, one lane per row. */
int ak_bpe_encode(const ak_bpe *m, ak_ws *ws, int flags, const uint8_t *in, const uint64_t *offs, uint64_t n,
                  uint32_t *ids, uint64_t cap, uint64_t *out_offs, uint8_t *row_status, void *stream);

/* aksharTokenizer(model, "sentencepiece").encode(text) (tokenizer.py:167-193): normalize_text then
 * EncodeAsIds (no bos/eos). */
int ak_spm_encode(const ak_spm *m, ak_ws *ws, int flags, const uint8_t *in, const uint64_t *offs, uint64_t n,
                  uint32_t *ids, uint64_t cap, uint64_t *out_offs, uint8_t *row_status, void *stream);

/* One string from host memory to host ids: aksharTokenizer.encode(text) as a non-Python caller binds
 * it (tokenizer.py:167-193; the FFI stub in INTEGRATION.md), for per-call latency. text: len UTF-8
 * bytes (host); ids: cap host int32 slots. The row goes through pinned staging in one
 * host->device copy, the same kernels as ak_bpe_encode / ak_spm_encode on `stream`, and one
 * device->host copy of count, error words and ids, with one stream synchronize (no read-backs in
 * between: the workspace knows the row's length). *n_ids = the id count; if it exceeds cap, nothing
 * is copied and the call returns AK_ERR_NOMEM (call again with a larger buffer). Synchronous: the
 * ids are in `ids` on return. */
int ak_bpe_encode_host(const ak_bpe *m, ak_ws *ws, int flags, const uint8_t *text, uint64_t len, int32_t *ids,
                       uint64_t cap, uint64_t *n_ids, void *stream);
int ak_spm_encode_host(const ak_spm *m, ak_ws *ws, int flags, const uint8_t *text, uint64_t len, int32_t *ids,
                       uint64_t cap, uint64_t *n_ids, void *stream);

/* Built-in kernel timing: when enabled, every batch call records HIP events around each of its
 * kernel launches on the caller's stream; ak_profile_read synchronizes the pending events and
 * returns the accumulated device time and launch count of one kernel class. */
#define AK_PROF_COUNT 0      /* fast count pass (one lane per row) */
#define AK_PROF_COUNT_SLOW 1 /* slow-path count pass (rows over the fast buffers) */
#define AK_PROF_SCAN 2       /* row counts -> row offsets (three small kernels) */
#define AK_PROF_EMIT 3       /* fast emit pass */
#define AK_PROF_EMIT_SLOW 4  /* slow-path emit pass */
#define AK_PROF_TILES 5      /* tile-cooperative BPE kernel (ids into per-unit staging runs) */
#define AK_PROF_COPY 6       /* staged ids -> final positions (tile path) */
#define AK_PROF_SPM_TILES 7  /* tile-cooperative SentencePiece kernel */
#define AK_PROF_ROW_TILES 8  /* tile-cooperative normalize / segment / switches / analyze kernel */
#define AK_PROF_FALLBACK_WAVE 9 /* fallback rows a wave each: SentencePiece redo, wave NFC + tile (BPE, SPM) */
#define AK_PROF_NKERNELS 10
/* level 0 off; 1 = HIP events around every launch (ak_profile_read; timing-neutral); 2 = also the
 * tile kernels' per-pass clocks (ak_profile_tile_passes), which instrument the kernels themselves */
int ak_profile_enable(int level);
int ak_profile_read(int kernel, double *total_ms, uint64_t *launches);
void ak_profile_reset(void);

/* Rows of the last tile-path ak_bpe_encode on this workspace that took the sequential fallback
 * kernels (NFC / HF-NFC quick check tripped, invalid UTF-8, or past the 768-byte tile buffer), and
 * how many of those needed the slow-tier pool buffers. Synchronizes the device. */
int ak_ws_fallback_rows(ak_ws *ws, uint64_t *rows, uint64_t *pool_rows);
/* The same launch in detail: [0] rows the tile kernel could not finish (SentencePiece: + the rows
 * a pooled word's margin test sent back); [1] of those, rows the tile path finished after all (NFC
 * by the fallback waves, k_bpe_nfc / k_spm_nfc; the send-backs re-encoded from the carried base by
 * k_spm_redo); [2] rows left to the one-lane row pipeline; [3] of those, rows that needed the
 * slow-tier buffers. A send-back row k_spm_redo passes on to the fallback list counts once.
 * Synchronizes. */
int ak_ws_fallback_detail(ak_ws *ws, uint64_t detail[4]);

/* Tile-kernel pass breakdown (profiling aid): device clock cycles summed over all waves for each
 * pass of the tile-cooperative BPE kernel since the last call, while profiling level 2 is on. Slots:
 * 0 byte staging, 1 decode + NFC check + map/filter, 2 fused elongation + HF NFKC + pre-tokenizer,
 * 3 pre-token cache probes, 4 pre-token start list, 5 BPE merges, 6 fallback-list append, 7 ids into the unit run +
 * counts, 8 (unused), 9 loop overhead.
 * Returns the number of slots written (0 if the tile kernel has not run), or a negative error. */
#define AK_TILE_NPASS 10
int ak_profile_tile_passes(ak_ws *ws, uint64_t *cycles, int n);
/* Event counters of the same instrumented launches (profiling level 2), reset by each call:
 * [0] BPE pre-tokens probed in the pre-token cache (slot 3 of the pass breakdown), [1] its hits,
 * [2] merge batches (64 pre-tokens a wave merges at once), [3] merge rounds, [4] lanes merging, summed
 * over rounds (lane utilisation of the merge loop = [4] / (64 [3])). SentencePiece launches: [0] / [1]
 * word-cache probes / hits, [2] word-pool batches, [3] rows redone from the carried base (in the tile,
 * or by the fallback kernels after a pooled word's margin test), [4] pooled words.
 * Returns the number of counters written (0 if no tile kernel has run), or a negative error. */
#define AK_TILE_NCOUNTERS 5
int ak_profile_tile_counters(ak_ws *ws, uint64_t *counts, int n);

/* Decode (tokenizer.py:195-219): rows of ids (u32, id_offs[n+1]) -> UTF-8 text
 * rows (out, out_offs[n+1]; out_offs[n] = required total even when cap is short).
 * ak_bpe_decode = HF Tokenizer.decode with the trained tokenizer.json (no decoder): special tokens
 * and ids outside the vocabulary are skipped, the other token strings joined by ' '. It needs the
 * vocabulary strings: ak_bpe_set_vocab (n ids, UTF-8 strings packed with tok_offs[n+1], special[n]
 * = 1 for special tokens; host pointers).
 * ak_spm_decode = SentencePieceProcessor.DecodeIds: control pieces vanish, <unk> -> " \u2047 ",
 * U+2581 -> ' ', <0xXX> byte runs reassembled as UTF-8 (invalid bytes -> U+FFFD each), leading
 * U+2581 dropped until the first non-empty piece; an id past the vocabulary is AK_ERR_ARG.
 * Device pointers; one wave per row. */
int ak_bpe_set_vocab(ak_bpe *m, uint32_t n, const uint8_t *tok_bytes, const uint64_t *tok_offs, const uint8_t *special);
int ak_bpe_decode(const ak_bpe *m, ak_ws *ws, const uint32_t *ids, const uint64_t *id_offs, uint64_t n, uint8_t *out,
                  uint64_t cap, uint64_t *out_offs, void *stream);
int ak_spm_decode(const ak_spm *m, ak_ws *ws, const uint32_t *ids, const uint64_t *id_offs, uint64_t n, uint8_t *out,
                  uint64_t cap, uint64_t *out_offs, void *stream);

/* Model-ready outputs from the ragged result of the encode calls (ids, id_offs[n+1] with id_offs[0] == 0,
 * as ak_bpe_encode / ak_spm_encode write them; `ids` needs no alignment). Device pointers; each call
 * is one kernel launch on `stream`, with no workspace and no read-back. Output arrays may be NULL
 * where marked optional. n == 0 and a capacity of 0 are allowed and store nothing. Argument errors
 * (NULL ids with n > 0, NULL id_offs, NULL out, width == 0 / block == 0, keep_head + keep_tail >
 * width, a flag bit the call does not take) are AK_ERR_ARG, found on the host before any device work.
 *
 * ak_ids_pad: out[n x width] (int32, or int64 with AK_DENSE_I64), row-major; what HF tokenizers'
 *   enable_truncation(width) + enable_padding(length=width, pad_id) give for a single-sequence template
 *   of keep_head leading and keep_tail trailing special tokens ("<s> $A </s>": 1 and 1). With L a row's
 *   length: L <= width keeps the row whole; L > width keeps its first keep_head ids, its last keep_tail
 *   ids and width - keep_head - keep_tail of the ids between them, the first ones, or the last ones
 *   with AK_TRUNC_LEFT. The other width - min(L, width) positions hold pad_id, after the ids, or before
 *   them with AK_PAD_LEFT. mask (optional, u8[n x width]): 1 for an id, 0 for padding; lengths (optional,
 *   int32[n]): min(L, width). An empty row is all padding. A row with 0 < L < keep_head + keep_tail is
 *   kept whole if L <= width, otherwise truncated as if keep_head = keep_tail = 0 (it cannot be longer than
 *   width, which is at least keep_head + keep_tail, so it is always kept whole). Nothing is stored at or
 *   past row cap_rows of out, mask or lengths.
 * ak_ids_pack: the rows concatenated, each followed by sep_id if sep_id >= 0 (S = 1, else S = 0), cut
 *   into blocks of `block` elements: row r takes stream positions [id_offs[r] + r S, id_offs[r+1] +
 *   (r+1) S), the total is T = id_offs[n] + n S, and out[n_blocks x block] (int32 / int64) has n_blocks =
 *   ceil(T / block), the positions from T on holding pad_id, or floor(T / block) with
 *   AK_PACK_DROP_LAST. pos (optional, int32, out's shape): the element's index inside its row (the
 *   separator included), counting on across block boundaries; 0 for padding. doc (optional, int32):
 *   the row index, -1 for padding; a row without elements (empty, S = 0) appears nowhere. Nothing is
 *   stored at or past block cap_blocks of out, pos or doc. id_offs[n] is read on the device:
 *   ak_ids_pack_blocks (host arithmetic) gives n_blocks for n_ids = id_offs[n] total ids. */
#define AK_PAD_LEFT 1       /* ak_ids_pad: padding before the ids */
#define AK_TRUNC_LEFT 2     /* ak_ids_pad: truncation keeps the last ids of the body */
#define AK_DENSE_I64 4      /* both: out is int64 */
#define AK_PACK_DROP_LAST 8 /* ak_ids_pack: no partial last block */
int ak_ids_pad(const int32_t *ids, const uint64_t *id_offs, uint64_t n, uint32_t width, int32_t pad_id,
               uint32_t keep_head, uint32_t keep_tail, int flags, void *out, uint64_t cap_rows, uint8_t *mask,
               int32_t *lengths, void *stream);
int ak_ids_pack(const int32_t *ids, const uint64_t *id_offs, uint64_t n, uint32_t block, int32_t sep_id,
                int32_t pad_id, int flags, void *out, int32_t *pos, int32_t *doc, uint64_t cap_blocks, void *stream);
uint64_t ak_ids_pack_blocks(uint64_t n_ids, uint64_t n, int has_sep, uint32_t block, int flags);

/* Sliding windows and text pairs: what HF tokenizers' enable_truncation(width, stride) gives with its
 * overflow encodings, for single sequences and for pairs. Input: a *sliding* stream (s_ids, s_offs[n+1])
 * and optionally a *fixed* stream (f_ids, f_offs[n+1]) with one partner row per sliding row, both as the
 * encode calls write them. A row has fewer than 2^32 ids (so have its windows: the counts are 32-bit).
 * keep_head = h / keep_tail = t are the template's special tokens inside every row, as in ak_ids_pad
 * ("<s> $A </s> <s> $B </s>": 1 and 1); a row shorter than h + t counts as h = t = 0. Per row, W = width:
 *   F'   the fixed row, cut to fixed_cap ids if it is longer, as ak_ids_pad truncates on the right
 *        (keeping h and t; a fixed_cap below h + t keeps the first fixed_cap ids); Lf' its length, 0
 *        without a fixed stream.
 *   C = W - Lf' - h - t ids of the sliding row's body (B ids) fit one window; consecutive windows start
 *        step = C - stride body ids apart. The row has 1 window if B <= C, else 1 + ceil((B - C) / step);
 *        an empty row has one too. Window k holds the row's h head ids, body[k step : min(k step + C, B)]
 *        and its t tail ids; the last window may be shorter than the others.
 *   The window's ids are F' then the sliding part (HF "only_second"), or the sliding part then F' with
 *   AK_WIN_FIXED_LAST ("only_first"), padded with pad_id to W on the right, or on the left with AK_PAD_LEFT.
 *   AK_WIN_LONGEST_FIRST (needs the fixed stream and stride == 0; fixed_cap is ignored): one window per
 *   row, the fixed row then the sliding row, their bodies cut to n1 and n2 ids by HF's rule: whole if
 *   they fit M = W - (h and t of both rows); else with n1 the shorter body and n2 the longer, n2 = n1 if
 *   n1 > M, else max(n1, M - n1); if still n1 + n2 > M, n1 = M / 2 and n2 = n1 + M % 2 (equal bodies: the
 *   fixed one is n1).
 * ak_ids_window_offs writes win_offs[n+1], the index of every row's first window (win_offs[n]: the
 * total; n == 0 writes win_offs[0] = 0). It uses the workspace and launches a count and a scan; there is
 * no read-back. ak_ids_windows takes the same arguments and that win_offs, and writes, in one launch:
 *   out       [n_windows x W] int32, or int64 with AK_DENSE_I64
 *   mask      (optional) u8, out's shape: 1 for an id, 0 for padding
 *   type_ids  (optional) u8, out's shape: 0 on the segment placed first and 1 on the one placed second,
 *             their special tokens included; 0 on padding and everywhere without a fixed stream
 *   sample    (optional) int32 [n_windows]: the window's row (HF overflow_to_sample_mapping)
 *   start     (optional) int32 [n_windows]: k step, the body index of the window's first body id
 *   lengths   (optional) int32 [n_windows]: ids in the window
 * Nothing is stored at or past window cap_windows. n == 0 and cap_windows == 0 store nothing and launch
 * nothing. AK_ERR_ARG, on the host before any device work: a NULL s_offs / win_offs / out / workspace,
 * NULL s_ids with n > 0, f_ids without f_offs or the reverse, width == 0, a flag bit other than
 * AK_PAD_LEFT | AK_DENSE_I64 | AK_WIN_* (AK_TRUNC_LEFT: windows slide rightwards only), fixed_cap != 0
 * without a fixed stream, width - fixed_cap - h - t <= stride (so step >= 1 for every row),
 * AK_WIN_LONGEST_FIRST without a fixed stream, with stride != 0, with width < 2 (h + t) or together with
 * AK_WIN_FIXED_LAST. */
#define AK_WIN_FIXED_LAST 16    /* the fixed segment follows the sliding one */
#define AK_WIN_LONGEST_FIRST 32 /* one window per row, the longer body cut first */
int ak_ids_window_offs(ak_ws *ws, const uint64_t *s_offs, const uint64_t *f_offs /*NULL: none*/, uint64_t n,
                       uint32_t width, uint32_t stride, uint32_t keep_head, uint32_t keep_tail, uint32_t fixed_cap,
                       int flags, uint64_t *win_offs, void *stream);
int ak_ids_windows(const int32_t *s_ids, const uint64_t *s_offs, const int32_t *f_ids, const uint64_t *f_offs,
                   uint64_t n, const uint64_t *win_offs, uint32_t width, uint32_t stride, uint32_t keep_head,
                   uint32_t keep_tail, uint32_t fixed_cap, int32_t pad_id, int flags, void *out,
                   uint64_t cap_windows, uint8_t *mask, uint8_t *type_ids, int32_t *sample, int32_t *start,
                   int32_t *lengths, void *stream);

/* Masked-LM batches (BERT's rule) from a dense id matrix, such as ak_ids_pad's: in, out and labels are
 * [rows x width], row-major, int32, or int64 with AK_DENSE_I64; device pointers with no alignment
 * requirement. One kernel launch on `stream`, no workspace, no read-back. Every step is unsigned
 * 32 / 64-bit integer arithmetic, so a call reproduces bit for bit:
 *   Element (r, c) has the 64-bit index e = elem_base + r width + c. Its draw is x0..x3 =
 *   Philox4x32-10(counter (lo32(e), hi32(e), lo32(stream_id), hi32(stream_id)), key (lo32(seed),
 *   hi32(seed))), with the published constants (multipliers 0xD2511F53, 0xCD9E8D57, Weyl increments
 *   0x9E3779B9, 0xBB67AE85; the all-zero counter and key give 6627e8d5 e169c58d bc57ac4c 9b00dbd8).
 *   An element is eligible when attn (optional, u8 [rows x width]) is NULL or attn[r, c] != 0, and its
 *   id is not one of never[0 .. n_never) (a host pointer, n_never <= 8).
 *   Leader: without word_start, the element itself. With word_start (optional, device, u8 [n_vocab]):
 *   the nearest (r, c') with c' <= c at which the run of eligible elements that holds c begins, or at
 *   which word_start[id] != 0; an id outside [0, n_vocab) counts as a word start. The search walks left
 *   inside row r only: it stops at column 0, at an ineligible element (the leader is the column after
 *   it) or at a flagged id.
 *   Selected: eligible and x0 of the leader's draw < t_select (compared in 64 bits: t_select = 2^32
 *   selects every eligible element).
 *   labels[r, c] = the input id if selected, else ignore_index. out[r, c] = the input id if not
 *   selected; if selected, by the element's own x1 and x2: mask_id if x1 < t_mask, else rand_lo +
 *   (int32)(((uint64)x2 (uint32)(rand_hi - rand_lo)) >> 32) if x1 < t_mask + t_random, else the input id.
 * Nothing is stored at or past row cap_rows. rows == 0 or cap_rows == 0 launches nothing. Calls over
 * parts of one batch draw what one call over the whole batch draws when elem_base is the part's first
 * element index. It works on ak_ids_pack's blocks as well, with sep_id and pad_id in never (a word or a
 * selection then never looks across a separator, but rows are blocks, not documents).
 * AK_ERR_ARG, on the host before any device work: NULL in, out or labels with rows > 0; width == 0; a
 * threshold above 2^32, or t_mask + t_random > 2^32; rand_hi <= rand_lo with t_random > 0; n_never > 8,
 * or never == NULL with n_never > 0; word_start with n_vocab == 0; a flag bit other than AK_DENSE_I64;
 * out or labels equal to in, or out == labels (the leader search reads neighbours: no in-place). */
int ak_ids_mlm(const void *in, const uint8_t *attn /*optional*/, uint64_t rows, uint32_t width, uint64_t seed,
               uint64_t stream_id, uint64_t elem_base, uint64_t t_select, uint64_t t_mask, uint64_t t_random,
               int32_t mask_id, int32_t rand_lo, int32_t rand_hi, int32_t ignore_index, const int32_t *never,
               uint32_t n_never, const uint8_t *word_start /*optional*/, uint32_t n_vocab, int flags, void *out,
               void *labels, uint64_t cap_rows, void *stream);

/* Span-corruption batches (T5's encoder-decoder objective) from a dense id matrix: `in` is [rows x width],
 * row-major, int32, or int64 with AK_DENSE_I64, as ak_ids_pack (full blocks: AK_PACK_DROP_LAST) or
 * ak_ids_pad write it; device pointers with no alignment requirement. One kernel launch on `stream`, no
 * workspace, no read-back. Every step is unsigned integer arithmetic, so a call reproduces bit for bit.
 *   Row r uses its first L = clamp(lengths[r], 0, width) ids (lengths: optional, device, int32 [rows];
 *   NULL: L = width). density_q32 in [0, 2^32] is the noise density times 2^32, mean_q16 >= 65536 the mean
 *   span length times 65536, E = 1 if eos_id >= 0, else 0.
 *   Counts: L < 2 gives N = S = 0 and M = L. Otherwise the row has
 *     N = clamp((L density_q32 + 2^31) >> 32, 1, L - 1) noise tokens, M = L - N kept tokens and
 *     S = clamp((2 N 65536 + mean_q16) / (2 mean_q16), 1, min(N, M)) spans (integer division);
 *   in_len = M + S + E and tgt_len = N + S + E. This is the arithmetic of T5's random_spans_noise_mask with
 *   round-half-up where Python's round() rounds half to even (a deliberate difference, as is the
 *   generator: T5 shuffles with its framework's, this draws keys with Philox).
 *   Draws: boundary j, 1 <= j < max(N, M), of row r has x0..x3 = Philox4x32-10 of the element index
 *   e = elem_base + r width + j, with ak_ids_mlm's counter and key layout (stream_id, seed). x0 is j's
 *   key in the noise segmentation (used for j < N), x1 its key in the non-noise one (j < M). In each
 *   segmentation the cuts are the S - 1 values of j with the smallest (key, j) pairs in lexicographic
 *   order (equal keys: the smaller j first): a uniformly random composition into S non-empty parts.
 *   Sorted, the noise cuts are a_1 < ... < a_(S-1) with a_0 = 0 and a_S = N; the others b_i, b_S = M.
 *   Layout: the row reads segment 0, span 0, segment 1, span 1, ...: it begins with kept tokens and ends
 *   with noise, as T5's does. Kept item v of segment i (b_i <= v < b_(i+1)) is column v + a_i; noise item
 *   u of span i (a_i <= u < a_(i+1)) is column u + b_(i+1). sentinel(i) = sentinel_first + i
 *   sentinel_step in wrapping int32 arithmetic (T5: the last vocabulary id and -1; sentinel_step = 0 with
 *   sentinel_first = <mask>: one <mask> per span, BART's text infilling).
 *   inputs  [rows x in_width], in's type:  inputs[r, v + i] = in[r, v + a_i]; inputs[r, b_(i+1) + i] =
 *           sentinel(i); inputs[r, M + S] = eos_id if E; pad_id from in_len on.
 *   targets [rows x tgt_width], in's type: targets[r, a_i + i] = sentinel(i); targets[r, u + i + 1] =
 *           in[r, u + b_(i+1)]; targets[r, N + S] = eos_id if E; tgt_pad_id from tgt_len on.
 *           L < 2 follows from N = S = 0: inputs hold the row's ids, then eos; targets eos alone.
 *   in_lengths / tgt_lengths (optional, int32 [rows]): in_len and tgt_len, what the row needs even where
 *           a width is shorter. noise (optional, u8 [rows x width]): 1 on noise columns, 0 on all others,
 *           those from L on included.
 * Ids travel at their full width (int64 ids outside int32 pass through); eos_id, the pads and the
 * sentinels are int32 values. Nothing is stored at or past column in_width / tgt_width of a row (an
 * element whose destination lies there is dropped) nor at or past row cap_rows. rows == 0 or cap_rows == 0
 * launches nothing. Calls over parts of one batch draw what one call over the whole batch draws when
 * elem_base is the part's first row times width. ak_ids_spans_lengths is the host arithmetic: out =
 * {N, S, in_len, tgt_len} for a row of L ids.
 * AK_ERR_ARG, on the host before any device work: NULL in, inputs or targets with rows > 0; width,
 * in_width or tgt_width == 0; width > AK_SPANS_MAX_WIDTH; density_q32 > 2^32; mean_q16 < 65536; a flag bit
 * other than AK_DENSE_I64; an output equal to in, to lengths or to another output; rows x the largest of
 * the three widths out of range; ak_ids_spans_lengths: NULL out, or the same two bounds. */
#define AK_SPANS_MAX_WIDTH 4096
int ak_ids_spans(const void *in, const int32_t *lengths /*optional*/, uint64_t rows, uint32_t width, uint64_t seed,
                 uint64_t stream_id, uint64_t elem_base, uint64_t density_q32, uint32_t mean_q16,
                 int32_t sentinel_first, int32_t sentinel_step, int32_t eos_id, int32_t pad_id, int32_t tgt_pad_id,
                 int flags, void *inputs, uint32_t in_width, void *targets, uint32_t tgt_width,
                 int32_t *in_lengths /*optional*/, int32_t *tgt_lengths /*optional*/, uint8_t *noise /*optional*/,
                 uint64_t cap_rows, void *stream);
int ak_ids_spans_lengths(uint32_t L, uint64_t density_q32, uint32_t mean_q16, int has_eos, uint64_t out[4]);

/* Always-sufficient output capacities (elements) for n rows of total_bytes input bytes.
 * ak_bpe_encode_cap holds for flags 2 / 3; with clean_hinglish=False (flags 0 / 1) NFKC can
 * expand a char (U+FDFA: 3 bytes -> 18 code points): AK_BPE_NFKC_EXPANSION * total_bytes + 2n + 16. */
#define AK_BPE_NFKC_EXPANSION 6
uint64_t ak_normalize_cap(uint64_t n, uint64_t total_bytes);
uint64_t ak_segment_cap(uint64_t n, uint64_t total_bytes);
uint64_t ak_bpe_encode_cap(uint64_t n, uint64_t total_bytes);
uint64_t ak_spm_encode_cap(uint64_t n, uint64_t total_bytes);

#ifdef __cplusplus
}
#endif
#endif /* AKSHAR_H */
