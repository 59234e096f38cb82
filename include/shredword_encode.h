/* shredword_encode.h — C ABI of the MI355X BPE encoder (libtrainer.so).
 *
 * Reads the trainer's on-disk formats and applies a trained merge list to text on the GPU.
 *   .model  M records of three native int32 (first, second, new_id = 256 + m), written by the
 *           reference's bpe_save (shredword/csrc/bpe/bpe.cpp:419-427);
 *   .vocab  256 + M records "<token bytes> <freq>\n" (bpe.cpp:416-418), token m = concatenation
 *           of its two operands' bytes (bpe.cpp:400-408).
 * The reference ships no loader or encoder for these files; the encoding is defined as the
 * trainer's own merge application replayed on new text: words are the maximal runs of bytes
 * outside "\t\r\n " (the strtok split of bpe.cpp:143-153), each byte becomes its symbol id
 * (bpe.cpp:154-180; bytes the trainer's coverage rule dropped become unk_id), and merge m is
 * applied to every word left to right without overlap (bpe.cpp:265-296) for m = 0, 1, ... .
 * Encoding the training corpus therefore reproduces the trainer's final segmentation, and the
 * per-id counts of the result equal the .vocab frequency column.
 *
 * Plain pointers and sizes only.  The handle owns device memory on one GPU; it is not
 * thread-safe.  Every entry point needs a HIP device: there is no CPU encoder.
 */
#ifndef SHREDWORD_ENCODE_H
#define SHREDWORD_ENCODE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Longest word an encoder in long-word mode accepts (bytes; shred_encoder_set_long_words below). */
#define SHRED_ENCODE_MAX_LONG_WORD (1u << 20)

typedef struct ShredEncoder ShredEncoder;

/* Longest word the encoder accepts (bytes); a longer word fails the call with -3, unless the
 * encoder's long-word mode is on (below). */
#define SHRED_ENCODE_MAX_WORD 1024

/* merges: num_merges triples (first, second, new_id) as in a .model file; new_id must be 256 + m
 * and first/second must be ids < new_id (or the call fails).  byte_map: 256 symbol ids (byte b
 * -> byte_map[b]) or NULL for the identity.  Returns NULL on invalid input or without a device
 * (the reason goes to stderr). */
ShredEncoder* shred_encoder_create(const int32_t* merges, size_t num_merges, const int32_t* byte_map,
                                   int device);

/* Loads a .model file.  With a .vocab path (may be NULL), bytes whose .vocab frequency is 0 and
 * that no merge uses map to unk_id (the trainer's coverage rule, recovered from its outputs);
 * without one the byte map is the identity. */
ShredEncoder* shred_encoder_load(const char* model_path, const char* vocab_path, int32_t unk_id, int device);

void shred_encoder_destroy(ShredEncoder* enc);

/* num_merges and the 256-entry byte map of an encoder (either pointer may be NULL). */
int shred_encoder_info(const ShredEncoder* enc, size_t* num_merges, int32_t* byte_map);

/* ---- words longer than SHRED_ENCODE_MAX_WORD ---------------------------------------------------
 *
 * Text without ASCII whitespace (CJK or Thai paragraphs, base64 blobs, minified code, long URLs)
 * holds words of any length.  By default such a word fails the call; with the long-word mode on it
 * is encoded, by a pass of its own in which one workgroup takes one word.  The ids are defined
 * exactly as for every other word (merge m applied left to right without overlap, for m = 0, 1,
 * ...), and nothing else about any output changes: word-begin rules, starts, line_off, row_off, the
 * byte map and the token lengths are as described below.
 *
 * Where the limit applies is unchanged: for shred_encode_special to the run before it is cut, for
 * shred_encode_docs to the words after the boundary cut.  The host calls keep cutting pieces after a
 * delimiter; a piece budget that falls inside a long word extends the piece to the end of that
 * word, which is staged whole (the rule a long document and a long row have).
 *
 * Cost.  With the mode off: none, and nothing is allocated.  With it on, every encode call reads
 * the text once more to find the long words (and waits for the count).  Scratch is allocated on the
 * first long word and freed with the encoder: 16 B per long word, 4 B per 32 text bytes, and, once
 * a word above 18432 bytes is met, 4 B per text byte.  A long word takes one round per distinct merge
 * rank that applies to it (at most min(num_merges, length - 1)), each round one pass of one
 * workgroup over the word's current tokens: natural text of 1 MB in one word took 1.6 s
 * under 7,936 merges, against 22 ms for 1 GB of ordinary text.
 */
/* on != 0: every encode call accepts words of up to SHRED_ENCODE_MAX_LONG_WORD bytes; words above
 * SHRED_ENCODE_MAX_WORD are encoded by the long-word pass.  -3 then means a word above the long
 * limit.  Default off.  Returns 0, -1 for NULL. */
int shred_encoder_set_long_words(ShredEncoder* enc, int on);
int shred_encoder_long_words(const ShredEncoder* enc);
/* What the long-word pass holds and has done (each pointer may be NULL): the bytes of device
 * scratch it has allocated (0 until a call meets a long word), the long words it has encoded and
 * the rounds it has run since the encoder was created.  Returns 0, -1 for NULL. */
int shred_encoder_long_stats(const ShredEncoder* enc, uint64_t* scratch_bytes, uint64_t* words, uint64_t* rounds);

/* ---- BPE-dropout: seeded subword regularisation (Provilkov et al. 2020) -----------------------------
 *
 * An encoder holds a dropout probability p in [0, 1] and a 64-bit seed; the default is p = 0.  With
 * p == 0 nothing below applies, and every call behaves, and is routed, as described elsewhere in this
 * file.  With p > 0, for every word of at most SHRED_ENCODE_MAX_WORD bytes:
 *
 *   - The tokens start as the byte-map ids of the word's bytes.
 *   - A candidate is an adjacent token pair (a, b) that the merge list knows; its rank is the first
 *     merge that lists the pair.
 *   - The candidate's position pos is the byte offset, in the text passed to the call, of the first
 *     byte of the right token b (a 64-bit value).
 *   - The candidate is dropped iff (u >> 32) < T, where
 *       mix(x):  x ^= x >> 33; x *= 0xff51afd7ed558ccd; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53;
 *                x ^= x >> 33   (mod 2^64: murmur3's fmix64),
 *       u = mix(mix(seed + 0x9E3779B97F4A7C15 * (pos + 1)) ^ rank),
 *       T = (uint64_t)(p * 4294967296.0), computed once in double arithmetic (p = 1: T = 2^32, every
 *           candidate is dropped and every non-delimiter byte keeps its byte-map id).
 *   - Repeat: among the candidates that are not dropped, merge the one of lowest rank, the leftmost on
 *     a tie.  Stop when none is left.
 *
 * A decision depends on (seed, pos, rank) alone: it is the same however often the loop meets that
 * candidate, independent of the neighbouring boundaries, and independent of how the text was staged.
 * This is the "drop a candidate once and for all" variant of BPE-dropout; it differs from the variants
 * that draw again at every merge step.  The same (text, p, seed) always gives the same ids, on host
 * and device calls alike; a new seed (per epoch, say) gives a new segmentation.  When p > 0 but
 * T == 0 (p < 2^-32) the call behaves as with p == 0.
 *
 * "The text passed to the call":
 *   shred_encode*, shred_encode_spans*, shred_encode_special*
 *       pos is the offset in `text`; the pieces of the host calls add their own offset.  The special
 *       calls encode a copy of the same length with the matches blanked, so the offsets are the
 *       text's; no merge reaches across a special, and the specials themselves are never dropped.
 *   shred_encode_docs*
 *       these encode a copy in which every document is followed by one inserted byte (below), and pos
 *       is the offset in that copy: for a byte of document d, its offset in the concatenated text
 *       plus d.
 * Everything behind the ids (starts, line_off, row_off, the special cut, decode, the batch calls)
 * follows from the ids' byte lengths and is defined as without dropout.
 *
 * Dropout reaches words of at most SHRED_ENCODE_MAX_WORD (1024) bytes.  In long-word mode a longer
 * word is encoded by the long-word pass exactly as without dropout; with the mode off it returns -3.
 *
 * Cost.  With p == 0: none, and nothing is allocated.  With p > 0 every call encodes each occurrence
 * of each word on its own (the word cache is neither filled nor read, since every occurrence differs;
 * such calls are not counted as cache fallbacks), and writes more ids.  Dropout's scratch (4 B per text
 * byte of the largest call) is allocated on the first dropout call and freed with the encoder.
 */
/* p in [0, 1]; p == 0 turns dropout off.  Returns 0; -1 for NULL, p < 0, p > 1 or NaN (the previous
 * setting stays). */
int shred_encoder_set_dropout(ShredEncoder* enc, double p, uint64_t seed);
/* The setting; either pointer may be NULL.  Returns 0, -1 for NULL. */
int shred_encoder_dropout(const ShredEncoder* enc, double* p, uint64_t* seed);

/* Encodes n bytes of host text into host ids.  Returns the number of ids written (<= the number
 * of non-delimiter bytes, so cap >= n always suffices), or -1 on a bad argument / device error,
 * -2 when cap is smaller than the result, -3 when a word exceeds SHRED_ENCODE_MAX_WORD (with the
 * long-word mode on: SHRED_ENCODE_MAX_LONG_WORD; so for every -3 below). */
int64_t shred_encode(ShredEncoder* enc, const uint8_t* text, size_t n, int32_t* out, size_t cap);

/* The same on device buffers (text: n bytes, out: cap >= n int32, both on the encoder's device),
 * queued on `stream` (a hipStream_t, NULL = the encoder's own) and synchronised before return.
 * The encoder's own stream is non-blocking: it is not ordered with the legacy default stream (the
 * handle 0, which therefore cannot be named here), so in every *_device call a caller with work
 * pending on that stream synchronises it first; the Python layer does (BPEEncoder._stream).
 * Same return values; kernel_ms (may be NULL) receives the device time of the encode passes. */
int64_t shred_encode_device(ShredEncoder* enc, const void* text, size_t n, void* out, size_t cap,
                            void* stream, double* kernel_ms);

/* Concatenates the bytes of n token ids into out (cap bytes).  Returns the byte count needed
 * (nothing is written past cap), or -1 for an id outside [0, 256 + num_merges + K), K the number
 * of registered special tokens (below).  Host only. */
int64_t shred_decode(const ShredEncoder* enc, const int32_t* ids, size_t n, uint8_t* out, size_t cap);

/* ---- token byte offsets and per-line id offsets ("offset mapping", dataset rows) ----------
 *
 * Ids come out in text order and no token spans a delimiter.  Id x covers len(x) source bytes:
 * 1 for an id below 256 (a byte's symbol; negative ids such as unk_id = -1 included), and
 * len(first[m]) + len(second[m]) for 256 + m.  The lengths follow from the merge list alone, so
 * they also hold for bytes the byte map sends to unk_id.  For a text of n bytes with T ids:
 *
 *   starts[k]    int64 byte offset in `text` of the first byte of token k; its end is
 *                starts[k] + len(ids[k]).  Token k begins a word iff k == 0 or
 *                starts[k] != starts[k-1] + len(ids[k-1]).
 *   lines        split on byte 10 only ('\r' is a word delimiter already, so CRLF text works):
 *                L = count('\n') + (n > 0 && text[n-1] != '\n').
 *   line_off     L + 1 int64 entries, line_off[0] = 0, line_off[L] = T; line i holds
 *                ids[line_off[i] : line_off[i+1]] for i in [0, L).  A line of only delimiters is
 *                an empty row.  n == 0 gives L = 0 and line_off = [0].
 *
 * The ids are exactly those of shred_encode on the same text.  The passes run on the GPU behind
 * the encode; their scratch (8 B per id + 32 B per 4096 text bytes) is allocated on the first
 * spans call and freed with the encoder, so shred_encode's footprint is unchanged.
 */

/* 256 + num_merges source-byte lengths (ids < 256: 1; saturating at INT32_MAX), then those of the
 * K registered special tokens (below).  Returns 0, or -1 when cap is smaller than 256 + num_merges
 * + K.  Host only. */
int shred_encoder_token_lengths(const ShredEncoder* enc, int32_t* out, size_t cap);

/* shred_encode plus, optionally, starts (NULL or cap int64) and line_off (NULL, or line_cap >=
 * lines + 1 int64).  *num_lines (may be NULL) receives L.  Returns the id count; -1/-2/-3 as
 * shred_encode, -2 also when line_cap is too small (then *num_lines holds the L that is needed
 * and nothing is written to line_off); -4 when the byte map holds an id >= 256 (a mapped byte
 * could not be told from a merged token, so lengths are undefined). */
int64_t shred_encode_spans(ShredEncoder* enc, const uint8_t* text, size_t n, int32_t* out, size_t cap,
                           int64_t* starts, int64_t* line_off, size_t line_cap, size_t* num_lines);

/* The same on device buffers; kernel_ms (NULL or 2 doubles): [0] the encode passes as in
 * shred_encode_device, [1] the span passes. */
int64_t shred_encode_spans_device(ShredEncoder* enc, const void* text, size_t n, void* out, size_t cap,
                                  void* starts, void* line_off, size_t line_cap, size_t* num_lines,
                                  void* stream, double* kernel_ms);

/* ---- special tokens matched in the text ----------------------------------------------------------
 *
 * An encoder holds an ordered list of K special tokens (control tokens such as "<|endoftext|>"),
 * each a byte string b_i.  Special i has id 256 + num_merges + i: the specials follow the merges
 * in the vocabulary, in the order given.  0 <= K <= SHRED_SPECIAL_MAX, 1 <= len(b_i) <=
 * SHRED_SPECIAL_MAX_LEN, all b_i distinct, and no b_i holds a delimiter byte ("\t\r\n "), so a
 * special always lies inside one word, never spans a line, and covers len(b_i) source bytes.
 *
 * Only the two shred_encode_special calls match them; every other encode call never does, whether
 * specials are registered or not (text from an untrusted source cannot inject control tokens
 * unless the caller asks).  Matching, within each maximal run of non-delimiter bytes, from the
 * run's first byte p on: if one or more specials equal text[p : p + len] and fit inside the run,
 * the longest is taken, its id is emitted and the scan continues at p + len; otherwise at p + 1
 * (leftmost, then longest, no overlap).  What remains of the run on either side of a match is
 * split into words as if the match were a delimiter, and those words are encoded as shred_encode
 * encodes them: no merge reaches across a special.  The word limit applies to the run before it
 * is cut: a run longer than SHRED_ENCODE_MAX_WORD fails the call with -3.
 *
 * starts[k] of a special is its match position, and the ids still tile the text's non-delimiter
 * bytes; lines and line_off are defined as above.  A special is a word of its own: token k begins
 * a word iff k == 0, or ids[k] or ids[k-1] is a special, or starts[k] != starts[k-1] +
 * len(ids[k-1]).  shred_encoder_token_lengths then holds 256 + num_merges + K entries.
 *
 * The decode calls below turn a special's id back into b_i (strict and unk mode alike); the
 * specials' bytes count towards SHRED_DECODE_MAX_VOCAB_BYTES.  The batch calls never look ids up.
 *
 * The passes run on the GPU around the encode.  Their scratch (5 B per text byte for the copy of
 * the text with the matches blanked and its word ids, 12 B per 32 text bytes of match counts, 8 B
 * per id, 12 B per match, the table of the specials) is allocated on the first special call and
 * freed with the encoder, so the other calls' footprints are unchanged.  A call that finds no
 * match costs one scan of the text on top of shred_encode_spans.
 */
#define SHRED_SPECIAL_MAX 256
#define SHRED_SPECIAL_MAX_LEN 64

/* Replaces the encoder's specials: special i is bytes[offsets[i] : offsets[i+1]] (K + 1 offsets);
 * K == 0 clears the set (bytes and offsets may then be NULL).  Returns 0, or -1 when a limit above
 * is violated; the previous set then stays in place. */
int shred_encoder_set_specials(ShredEncoder* enc, const uint8_t* bytes, const size_t* offsets, size_t K);

size_t shred_encoder_num_specials(const ShredEncoder* enc);

/* shred_encode_spans with the registered specials matched: the same arguments, NULL rules and
 * return values, and the same staging in pieces (a special never straddles two pieces).  With
 * K == 0 it returns exactly what shred_encode_spans returns. */
int64_t shred_encode_special(ShredEncoder* enc, const uint8_t* text, size_t n, int32_t* out, size_t cap,
                             int64_t* starts, int64_t* line_off, size_t line_cap, size_t* num_lines);

/* The same on device buffers, as shred_encode_spans_device; kernel_ms (NULL or 3 doubles): [0] the
 * encode passes, [1] the span passes, [2] the special passes. */
int64_t shred_encode_special_device(ShredEncoder* enc, const void* text, size_t n, void* out, size_t cap,
                                    void* starts, void* line_off, size_t line_cap, size_t* num_lines,
                                    void* stream, double* kernel_ms);

/* ---- batches of documents: rows cut at given byte offsets ------------------------------------------
 *
 * The calls above take one text and know rows only as '\n' lines.  These take many documents in
 * one call, and their rows are the documents, which may hold '\n' themselves.
 *
 *   text       n bytes: the documents concatenated with nothing between them.
 *   doc_off    docs + 1 int64 with 0 = doc_off[0] <= ... <= doc_off[docs] = n; any other doc_off
 *              returns -6 with nothing written.  Document d is text[doc_off[d] : doc_off[d+1]] and
 *              may be empty.  NULL with docs == 0: one document holding all of text (the outputs
 *              then have 1 row and row_off 1 + 1 entries, the row_off == NULL rule of the decode
 *              and batch calls).  rows below is docs, or 1 for doc_off == NULL.
 *
 * Each document is encoded as if alone: a document boundary is a zero-width delimiter, and no
 * word, no merge and no special-token match reaches across it.  '\n' inside a document is an
 * ordinary delimiter, as in shred_encode.
 *
 *   ids        shred_encode(doc_0) ++ shred_encode(doc_1) ++ ...; with specials != 0 each part is
 *              shred_encode_special(doc_d) instead (exactly shred_encode's when K == 0).
 *   row_off    rows + 1 int64 in the line_off format: row_off[0] = 0, row_off[rows] = T, row d is
 *              ids[row_off[d] : row_off[d+1]].  An empty or all-delimiter document is an empty row.
 *              It feeds shred_pad_*, shred_pack_* and shred_decode_* unchanged.  Must not be NULL.
 *   starts     NULL, or cap int64: byte offsets in the concatenated text, not relative to the
 *              document.  The ids still tile the non-delimiter bytes of text in order.  Token k
 *              begins a word iff k == 0, or k is the first token of its row, or ids[k] or ids[k-1]
 *              is a special, or starts[k] != starts[k-1] + len(ids[k-1]).
 *
 * The word limit applies to the words after the cut: a run of 2000 non-delimiter bytes that a
 * boundary cuts into 1000 + 1000 passes, a document holding a run of SHRED_ENCODE_MAX_WORD + 1
 * returns -3.  Returns the id count T; -1 / -2 / -3 / -4 as shred_encode_spans (-4 because the rows
 * are found from the tokens' byte lengths), -6 as above.  On any error row_off and starts are not
 * written.  (A HIP error after the first piece of shred_encode_docs leaves the earlier pieces'
 * entries in place.)
 *
 * The passes run on the GPU around the encode: a copy of the text in which every document is
 * followed by one '\n' and holds none itself (its own become ' ', a delimiter too), the encode and
 * the span passes on that copy (whose lines are the documents), and a pass that takes the inserted
 * bytes out of starts.  Their scratch (1 B per text byte + 1 B per document for the copy, a flag
 * word, events) is allocated on the first docs call and freed with the encoder, so the other
 * calls' footprints are unchanged; the encode and span scratch is that of shred_encode_spans on
 * n + docs bytes, with specials that of shred_encode_special.
 */

/* Host buffers, staged through cached device buffers in pieces that hold whole documents: a piece
 * takes documents while their bytes plus one per document stay within the piece budget of
 * shred_encode.  A single document longer than a piece is staged whole (the rule shred_pad_rows
 * has for a long row): the longest document bounds the device memory.  Staging: 13 B per piece
 * byte (text, ids, starts) + 16 B per document of the piece.  doc_off is validated, and the word
 * limit checked, on the host before anything is staged; when cap is smaller than the text's
 * non-delimiter bytes, a first round of the pieces only counts the ids, so -2 too comes before
 * anything is written. */
int64_t shred_encode_docs(ShredEncoder* enc, const uint8_t* text, size_t n, const int64_t* doc_off, size_t docs,
                          int specials, int32_t* out, size_t cap, int64_t* starts, int64_t* row_off);

/* All buffers on the encoder's device; doc_off is validated there (a flag word the host reads
 * before any other pass runs).  Queued on `stream` (NULL = the encoder's own) and synchronised
 * before return.  kernel_ms (NULL or 4 doubles): [0] the encode passes, [1] the span passes, [2]
 * the special passes, [3] the document passes. */
int64_t shred_encode_docs_device(ShredEncoder* enc, const void* text, size_t n, const void* doc_off, size_t docs,
                                 int specials, void* out, size_t cap, void* starts, void* row_off, void* stream,
                                 double* kernel_ms);

/* ---- ids back to bytes on the GPU, per row ---------------------------------------------------
 *
 *   ids        n int32.
 *   row_off    NULL with rows == 0: one row holding all ids.  Otherwise rows + 1 int64 entries in
 *              the line_off format above: row_off[0] == 0, non-decreasing, row_off[rows] == n;
 *              row r holds ids[row_off[r] : row_off[r+1]].  Empty rows are allowed.
 *   sep        -1 for none, or a byte 0..255 written after every row, the last and empty rows
 *              included (with row_off == NULL one separator ends the single row).  line_off from
 *              shred_encode_spans with sep = '\n' gives one '\n'-terminated line per row.
 *   unk        the vocabulary is [0, 256 + num_merges + K) with K registered special tokens.
 *              unk_len == -1 is strict: an id outside the vocabulary fails the call with
 *              -1, as shred_decode does.  0 <= unk_len <= SHRED_DECODE_MAX_UNK: each such id
 *              decodes to these unk_len bytes (0 drops it).
 *   byte_off   NULL, or rows + 1 int64 (1 + 1 when row_off is NULL): byte_off[r] is the offset in
 *              out of row r's first byte, byte_off[rows] the total.  Row r without its separator
 *              is out[byte_off[r] : byte_off[r+1] - (sep >= 0)].
 *
 * Returns the byte count needed.  If out is NULL or cap is smaller than that, nothing is written
 * to out or byte_off (the sizing call: only the length passes run); otherwise exactly that many
 * bytes are written and nothing past them.  Errors, with nothing written to out or byte_off:
 * -1 bad argument, unk_len out of range, HIP error, or a strict-mode id outside the vocabulary;
 * -5 the vocabulary's bytes exceed SHRED_DECODE_MAX_VOCAB_BYTES; -6 row_off is not
 * 0 = row_off[0] <= ... <= row_off[rows] = n.  (A HIP error after the first piece of
 * shred_decode_rows leaves the earlier pieces' bytes in out.)
 *
 * The vocabulary (4 B per id + its bytes) and the decode scratch (12 B per id, 16 B with rows and
 * a separator) are allocated on the first decode call and freed with the encoder, so the encode
 * calls' footprints are unchanged.
 */

/* All buffers on the encoder's device (row_off is validated there); queued on `stream` (NULL =
 * the encoder's own) and synchronised before return.  kernel_ms (may be NULL) receives the
 * device time of the decode passes. */
int64_t shred_decode_device(ShredEncoder* enc, const void* ids, size_t n, const void* row_off, size_t rows,
                            void* out, size_t cap, void* byte_off, int sep, const uint8_t* unk, int unk_len,
                            void* stream, double* kernel_ms);

/* Host buffers, staged through cached device buffers in pieces of a fixed number of ids (cut at
 * any id, so rows straddle pieces): device memory does not grow with n. */
int64_t shred_decode_rows(ShredEncoder* enc, const int32_t* ids, size_t n, const int64_t* row_off, size_t rows,
                          uint8_t* out, size_t cap, int64_t* byte_off, int sep, const uint8_t* unk, int unk_len);

/* ---- rows of ids to rectangular model inputs on the GPU: padded batches, packed sequences ------
 *
 * Inputs of both forms:
 *   ids         n int32.
 *   row_off     rows + 1 int64 in the line_off format: 0 = row_off[0] <= ... <= row_off[rows] = n,
 *               else the call returns -6.  NULL with rows == 0: all ids form one row (the outputs
 *               below then have 1 row, and row_start 1 + 1 entries).  len_r = row_off[r+1] - row_off[r].
 *   bos, eos    each NULL for none, or a host pointer to one int32 id.  Any int32 value is allowed:
 *               the ids are never looked up in the vocabulary.  add = (bos != NULL) + (eos != NULL).
 *   max_len     0: unlimited.  Otherwise every emitted row holds at most max_len ids, the added
 *               ones included; max_len < add returns -1.
 *               keep_r = len_r when unlimited, else min(len_r, max_len - add).
 *   trunc_side  0 keeps the first keep_r ids of a row, 1 the last keep_r.
 *
 * Emitted row r is [bos] + kept ids + [eos], of length e_r = add + keep_r.  E[r] is the sum of
 * e_r' over r' < r, E[rows] = T.  An empty row emits only its added ids; with add == 0 it emits
 * nothing, so E repeats a value.
 *
 * Pad (width = W, pad_id, pad_side): out is [rows, W] int32, row-major.
 *   pad_side 0  out[r, c] = emitted id c for c < e_r, else pad_id.
 *   pad_side 1  emitted id j goes to out[r, W - e_r + j]; everything to its left is pad_id.
 *   lengths     NULL, or rows int32: lengths[r] = e_r.
 *   mask        NULL, or [rows, W] uint8: 1 where a token sits, 0 where padding sits.
 *   Returns max_r e_r (0 for rows == 0).  Nothing is written if out is NULL, or width is smaller
 *   than that, or cap < rows * width (cap counts int32 entries): the sizing call, only the length
 *   passes run.  With max_len > 0, width = max_len always suffices.
 *
 * Pack (seq_len = L >= 1, pad_id, drop_last): the stream is the concatenation of the emitted rows.
 *   S = ceil(T / L), or floor(T / L) with drop_last.  out is [S, L] int32, row-major:
 *   out[p] = stream id p for p < min(T, S * L), and pad_id for T <= p < S * L (a tail that exists
 *   only without drop_last).
 *   pos         NULL, or S * L int32: the index of p inside its emitted row (a bos is at 0);
 *               padding gets 0.
 *   seg         NULL, or S * L int32: the row index r; padding gets -1.  rows > INT32_MAX returns -1.
 *   row_start   NULL, or rows + 1 int64: E[0 .. rows], written in full even when drop_last cuts
 *               the stream.
 *   Returns S.  Nothing is written if out is NULL or cap < S * L.
 *
 * Errors of both, with nothing written: -1 bad argument, HIP error, or an e_r, rows * width or
 * S * L that does not fit its type (int32, size_t / int64); -6 bad row_off.  (A HIP error after
 * the first piece of the _rows calls leaves the earlier pieces' output in place.)
 *
 * The batch scratch (8 B per row for E, the scan's temporaries, a pinned result word, events) is
 * allocated on the first batch call and freed with the encoder, so the encode and decode calls'
 * footprints are unchanged.
 */

/* All buffers on the encoder's device (row_off is validated there); queued on `stream` (NULL =
 * the encoder's own) and synchronised before return.  Output pointers need only their element's
 * alignment (4 bytes; 1 for mask), so tensor views fit.  kernel_ms (may be NULL) receives the
 * device time of the batch passes. */
int64_t shred_pad_device(ShredEncoder* enc, const void* ids, size_t n, const void* row_off, size_t rows,
                         const int32_t* bos, const int32_t* eos, size_t max_len, int trunc_side, size_t width,
                         int32_t pad_id, int pad_side, void* out, size_t cap, void* lengths, void* mask,
                         void* stream, double* kernel_ms);
int64_t shred_pack_device(ShredEncoder* enc, const void* ids, size_t n, const void* row_off, size_t rows,
                          const int32_t* bos, const int32_t* eos, size_t max_len, int trunc_side, size_t seq_len,
                          int32_t pad_id, int drop_last, void* out, size_t cap, void* pos, void* seg,
                          void* row_start, void* stream, double* kernel_ms);

/* Host buffers, staged through cached device buffers in pieces cut at row boundaries: a piece
 * takes whole rows while it holds at most a fixed number of ids (and of rows, and for pad of
 * output entries), so device memory does not grow with n.  A single row longer than a piece is
 * staged whole: the longest row bounds the device memory.  Without row_off the one row is one piece. */
int64_t shred_pad_rows(ShredEncoder* enc, const int32_t* ids, size_t n, const int64_t* row_off, size_t rows,
                       const int32_t* bos, const int32_t* eos, size_t max_len, int trunc_side, size_t width,
                       int32_t pad_id, int pad_side, int32_t* out, size_t cap, int32_t* lengths, uint8_t* mask);
int64_t shred_pack_rows(ShredEncoder* enc, const int32_t* ids, size_t n, const int64_t* row_off, size_t rows,
                        const int32_t* bos, const int32_t* eos, size_t max_len, int trunc_side, size_t seq_len,
                        int32_t pad_id, int drop_last, int32_t* out, size_t cap, int32_t* pos, int32_t* seg,
                        int64_t* row_start);

/* ---- long rows cut into overlapping windows on the GPU ("overflowing tokens with a stride") --------
 *
 * Pad with max_len keeps one end of a long row; these keep all of it, as several rows of the batch
 * that still belong to the input row.  ids, row_off / rows (the NULL / rows == 0 rule, -6), bos, eos
 * and add are those of the batch calls above.
 *   max_len     required: every window holds at most max_len ids, the added ones included, so
 *               C = max_len - add ids of its row.  1 <= C and max_len <= INT32_MAX, else -1.
 *   stride      consecutive windows of a row share exactly stride ids: window j starts
 *               step = C - stride ids after window j - 1.  0 <= stride < C, else -1.
 *
 * Row r of len_r ids has w_r = 1 windows if len_r <= C, else 1 + ceil((len_r - C) / step).  Window j
 * holds the row's ids [j * step, min(j * step + C, len_r)) and is emitted as [bos] + those ids +
 * [eos], of length e = add + their count: only a row's last window can be shorter than max_len.
 * An empty row has one window that holds only the added ids (with add == 0: only padding), so
 * every input row is represented, as in pad.  WO[r] is the sum of w_r' over r' < r, Wn = WO[rows].
 * There is no trunc_side: nothing is dropped.
 *
 * Outputs (width = W, pad_id, pad_side as in pad); all but out may be NULL:
 *   out         [Wn, W] int32, row-major: window w as pad writes an emitted row.
 *   lengths     Wn int32: e of each window.
 *   mask        [Wn, W] uint8: 1 where a token sits, 0 where padding sits.
 *   win_row     Wn int32: the row r of each window.  rows > INT32_MAX returns -1 when it is asked for.
 *   win_src     Wn int64: the index in ids of the window's first kept id, row_off[r] + j * step.  The
 *               kept id at emitted position c in [bos != NULL, e - (eos != NULL)) is
 *               ids[win_src[w] + c - (bos != NULL)], and the same index into starts (shred_encode_spans,
 *               shred_encode_docs) is that token's byte offset: the offset mapping of a window.
 *   row_win     rows + 1 int64 (1 + 1 when row_off is NULL): WO[0 .. rows]; row r owns the windows
 *               [row_win[r], row_win[r+1]).
 *   widest      NULL, or a host size_t that receives the largest e (0 for rows == 0).
 *
 * Returns Wn.  Nothing is written but *widest if out is NULL, or width is smaller than *widest, or
 * cap < Wn * width (cap counts int32 entries): the sizing call, only the length passes run.
 * width = max_len always suffices.  Errors, with nothing written at all: -1 bad argument, HIP
 * error, or a Wn * width that does not fit an int64; -6 bad row_off.  (A HIP error after the first
 * piece of shred_window_rows leaves the earlier pieces' output in place.)
 *
 * The window scratch (8 B per row for WO, the scan's temporaries, a pinned result word, events) is
 * allocated on the first window call and freed with the encoder, so the other calls' footprints
 * are unchanged.
 */

/* All buffers on the encoder's device (row_off is validated there); stream, alignment and
 * kernel_ms as shred_pad_device. */
int64_t shred_window_device(ShredEncoder* enc, const void* ids, size_t n, const void* row_off, size_t rows,
                            const int32_t* bos, const int32_t* eos, size_t max_len, size_t stride, size_t width,
                            int32_t pad_id, int pad_side, void* out, size_t cap, void* lengths, void* mask,
                            void* win_row, void* win_src, void* row_win, size_t* widest, void* stream,
                            double* kernel_ms);

/* Host buffers; row_off, Wn and the widest window are settled on the host before anything is
 * staged.  Staged like shred_pad_rows in pieces of whole rows: a piece takes rows while its ids,
 * its rows and its output entries (windows * width, at most 4 per id of the budget) stay within
 * the piece budget, and one row is taken whole, however long.  A piece writes its own windows of
 * every output. */
int64_t shred_window_rows(ShredEncoder* enc, const int32_t* ids, size_t n, const int64_t* row_off, size_t rows,
                          const int32_t* bos, const int32_t* eos, size_t max_len, size_t stride, size_t width,
                          int32_t pad_id, int pad_side, int32_t* out, size_t cap, int32_t* lengths, uint8_t* mask,
                          int32_t* win_row, int64_t* win_src, int64_t* row_win, size_t* widest);

/* ---- row pairs to one model input on the GPU: two segments, one budget, token types ---------------
 *
 * The calls above take one row per example.  These take two (question and context, premise and
 * hypothesis, prompt and response) and emit [bos] + kept_a + mid + kept_b + [eos].
 *
 * Inputs:
 *   ids_a, row_a   n_a int32 with rows + 1 int64 offsets; ids_b, row_b: n_b int32 with rows + 1 int64
 *               offsets.  Both offset arrays are in the line_off format (0 = row[0] <= ... <=
 *               row[rows] = n, else -6) and neither may be NULL; they share the one row count.
 *               Example r has la_r = row_a[r+1] - row_a[r] ids of a and lb_r ids of b.
 *   bos, eos    each NULL for none, or a host pointer to one int32 id.
 *   mid, mid_n  0 <= mid_n <= 2 ids between the segments (a host pointer; RoBERTa uses two).  Like
 *               bos and eos they may be any int32 and are never looked up.
 *               add = (bos != NULL) + mid_n + (eos != NULL).
 *   max_len     0: unlimited, allowed for strategies 0 .. 2 only.  Otherwise B = max_len - add is the
 *               budget of kept ids per emitted row; max_len < add returns -1.
 *   trunc_side  0 keeps the first ids of a segment that is cut, 1 its last.
 *   strategy    how a pair is made to fit, below; max_a and stride go with strategy 3 and must be 0
 *               with the others.
 *
 * An emitted row is [bos] + kept_a + mid + kept_b + [eos], of length e = add + ka + kb.  Token
 * types: bos, kept_a and mid have type 0, kept_b and eos type 1, padding type 0.
 *
 *   0  longest_first   while ka + kb > B, remove one id from the longer segment, from b on a tie.
 *                      In closed form, with s = min(la, lb): if la + lb <= B both stay whole; else if
 *                      2 s <= B the shorter stays whole and the longer keeps B - s; else
 *                      ka = ceil(B / 2), kb = floor(B / 2).
 *   1  only_first      kb = lb, ka = min(la, B - lb).  An example with lb > B cannot fit.
 *   2  only_second     ka = la, kb = min(lb, B - la).  An example with la > B cannot fit.
 *   3  window_second   the question-answering form; needs 0 < max_len <= INT32_MAX.  ka = la when
 *                      max_a == 0, else min(la, max_a), cut on trunc_side.  b is never dropped: it is
 *                      cut into windows of C_r = B - ka_r ids, step_r = C_r - stride apart, by the
 *                      rule of shred_window_* (w_r = 1 if lb_r <= C_r, else 1 + ceil((lb_r - C_r) /
 *                      step_r); window j holds the ids [j step_r, min(j step_r + C_r, lb_r)) of b; an
 *                      empty b has one window).  Every window of example r carries the same kept_a.
 *                      An example with C_r < stride + 1 cannot fit (ka_r > B included).  With
 *                      max_a > 0 the call checks B - max_a >= stride + 1 once (-1), and then no
 *                      example can fail.
 *
 * -7: some example cannot be made to fit by the strategy; nothing is written.  The device call finds
 * it in its row pass, the host call before anything is staged.
 *
 * w_r is the number of emitted rows of example r (1 for strategies 0 .. 2), WO[r] the sum of w_r' over
 * r' < r, Wn = WO[rows].  An example with both rows empty emits only the added ids (with add == 0:
 * only padding), so every example is represented, as in pad and window.
 *
 * Outputs (width = W, pad_id, pad_side as in pad); all but out may be NULL:
 *   out         [Wn, W] int32, row-major: emitted row w as pad writes an emitted row.
 *   types       [Wn, W] uint8: the token types above.
 *   mask        [Wn, W] uint8: 1 where a token sits, 0 where padding sits.
 *   lengths     Wn int32: e of each emitted row.
 *   win_row     Wn int32: the example r.  rows > INT32_MAX returns -1 when it is asked for.
 *   seg_len     [Wn, 2] int32: (ka, kb) of the emitted row.
 *   seg_src     [Wn, 2] int64: the index in ids_a of the first kept a id and the index in ids_b of the
 *               first kept b id (for a segment that keeps nothing: the index at which it would begin).
 *   row_win     rows + 1 int64: WO[0 .. rows]; example r owns the emitted rows [row_win[r], row_win[r+1]).
 *   widest      NULL, or a host size_t that receives the largest e (0 for rows == 0).
 *
 * With bos_n = (bos != NULL): kept_a sits at the emitted positions [bos_n, bos_n + ka), and position c
 * there holds ids_a[seg_src[w][0] + c - bos_n]; kept_b sits at [bos_n + ka + mid_n, bos_n + ka + mid_n
 * + kb), and position c there holds ids_b[seg_src[w][1] + c - (bos_n + ka + mid_n)].  The same two
 * indices into the starts arrays that shred_encode_docs returns for the two texts are those tokens'
 * byte offsets: the offset mapping of a pair.
 *
 * Returns Wn.  Nothing is written but *widest if out is NULL, or width is smaller than *widest, or
 * cap < Wn * width (cap counts int32 entries): the sizing call, only the length passes run.  With
 * max_len > 0, width = max_len always suffices.  Errors, with nothing written at all: -1 bad
 * argument (an unknown strategy; stride or max_a given with strategies 0 .. 2; strategy 3 without a
 * max_len), HIP error, an e above INT32_MAX, or a Wn * width that does not fit an int64; -6 a bad
 * row_a or row_b; -7 as above (-6 comes before -7, and -7 before an e above INT32_MAX).  (A HIP error
 * after the first piece of shred_pair_rows leaves the earlier pieces' output in place.)
 *
 * The pair scratch (8 B per example for WO, the scan's temporaries, a pinned result word, events,
 * and the host call's staging) is allocated on the first pair call and freed with the encoder, so
 * the other calls' footprints are unchanged.
 */

/* All buffers on the encoder's device (row_a and row_b are validated there); stream, alignment
 * (4 bytes; 1 for types and mask; 8 for the int64 outputs) and kernel_ms as shred_pad_device. */
int64_t shred_pair_device(ShredEncoder* enc, const void* ids_a, size_t n_a, const void* row_a, const void* ids_b,
                          size_t n_b, const void* row_b, size_t rows, const int32_t* bos, const int32_t* mid,
                          size_t mid_n, const int32_t* eos, size_t max_len, int trunc_side, int strategy, size_t max_a,
                          size_t stride, size_t width, int32_t pad_id, int pad_side, void* out, size_t cap, void* types,
                          void* mask, void* lengths, void* win_row, void* seg_len, void* seg_src, void* row_win,
                          size_t* widest, void* stream, double* kernel_ms);

/* Host buffers; the offset arrays, the examples that cannot fit, Wn and the widest emitted row are
 * settled on the host before anything is staged.  Staged like shred_window_rows in pieces of whole
 * examples: a piece takes examples while its ids of a plus its ids of b, its examples and its output
 * entries (emitted rows * width, at most 4 per id of the budget) stay within the piece budget of the
 * batch calls, and one example is taken whole, however long.  A piece writes its own emitted rows of
 * every output. */
int64_t shred_pair_rows(ShredEncoder* enc, const int32_t* ids_a, size_t n_a, const int64_t* row_a, const int32_t* ids_b,
                        size_t n_b, const int64_t* row_b, size_t rows, const int32_t* bos, const int32_t* mid,
                        size_t mid_n, const int32_t* eos, size_t max_len, int trunc_side, int strategy, size_t max_a,
                        size_t stride, size_t width, int32_t pad_id, int pad_side, int32_t* out, size_t cap,
                        uint8_t* types, uint8_t* mask, int32_t* lengths, int32_t* win_row, int32_t* seg_len,
                        int64_t* seg_src, int64_t* row_win, size_t* widest);

/* ---- masked-LM inputs on the GPU: per token or per whole word -------------------------------------
 *
 * The masked-language-model objective (BERT / RoBERTa pre-training, ELECTRA generators) selects some
 * tokens, replaces most of them, and asks the model for the originals.  These calls work on the flat
 * (ids, row_off) pair, before pad, pack, window or pair, and so compose with all four: the caller pads
 * the masked ids as usual and pads the labels with pad_id = bos = eos (= mid) = ignore_id, which the
 * batch calls allow because they never look ids up.  Truncation and windowing then agree between the
 * two, because both use the same row_off.
 *
 * Inputs:
 *   ids         n int32.
 *   row_off     the usual rows + 1 int64, or NULL with rows == 0 for one row; validated as elsewhere (-6).
 *   starts      with whole_word != 0: n int64, as shred_encode_spans / shred_encode_docs return them
 *               (NULL with n > 0 then returns -1).  Not read otherwise, and may be NULL.
 *   opts        the scalar options, ShredMlmOpts below:
 *     index_base        uint64 added to every index below.  The host call's pieces use it; a caller
 *                       sharding a stream over calls may use it too.
 *     p, seed           selection probability in [0, 1] and a 64-bit seed.
 *     p_mask, p_random  of the selected tokens: the share replaced by mask_id, and the share replaced
 *                       by a random id.  The rest keep their id.  Both lie in [0, 1] and their sum is
 *                       at most 1.
 *     mask_id           any int32.
 *     rand_vocab        random replacements are uniform in [0, rand_vocab).  Required in
 *                       [1, INT32_MAX] when p_random > 0.
 *     protect, protect_n  host pointer to at most SHRED_MLM_MAX_PROTECT int32 ids that are never
 *                       selected (unk, a pad id already present, and so on).
 *     protect_specials  non-zero: the K registered specials (ids in [256 + M, 256 + M + K)) are never
 *                       selected either.
 *     whole_word        non-zero: tokens are selected by whole words.
 *     ignore_id         label of every token not selected.  Callers pass -100.
 *
 * Definitions, with mix = fmix64 exactly as in the dropout section and G = 0x9E3779B97F4A7C15:
 *   d(x, c) = mix(mix(seed + G * (x + 1)) ^ c), with the constants SEL = 1 << 40 and
 *             ACT = (1 << 40) + 1.  They are above every merge rank, so the same seed used for
 *             dropout and for masking gives unrelated draws.
 *   T(q)    = (uint64_t)(q * 4294967296.0), computed in double.  T(p_mask) + T(p_random) > 2^32
 *             returns -1.
 *   Unit of token k: without whole_word, h(k) = index_base + k.  With it, h(k) = index_base + k',
 *             where k' is the largest k' <= k at which a word begins.  A word begins by the rule of
 *             the sections above, with one addition.  Token k begins a word iff
 *               k == 0, or k is the first token of its row, or
 *               ids[k] or ids[k-1] is a registered special, or
 *               starts[k] != starts[k-1] + len(ids[k-1]), where len is that of the token-lengths
 *               table (1 for ids below 256, for negative ids and for ids past the table), or
 *               ids[k] or ids[k-1] is protected (the protect list, and the specials under
 *               protect_specials).  This is the addition: a protected id is a unit of its own.
 *   Token k is selected iff ids[k] is not protected and (d(h(k), SEL) >> 32) < T(p).  All
 *             unprotected tokens of a word therefore fall together.
 *   For a selected token, let a = d(index_base + k, ACT) and v = a >> 32.
 *             If v < T(p_mask):                    out[k] = mask_id.
 *             Else if v < T(p_mask) + T(p_random): out[k] = (int32)(((a & 0xFFFFFFFF) * rand_vocab) >> 32).
 *             Else                                 out[k] = ids[k].
 *             labels[k] = ids[k].  The action is drawn per token, also inside a whole word.
 *   A token not selected has out[k] = ids[k] and labels[k] = ignore_id.
 *
 * A decision depends on (seed, index, ids, starts) alone: the same arguments give the same result on
 * host and device calls alike and for every staging, and a new seed (per epoch, say) a new masking.
 *
 * Returns the number of selected tokens.  Errors, with nothing written: -1 bad argument (a
 * probability outside [0, 1] or NaN, T(p_mask) + T(p_random) > 2^32, protect_n above the limit,
 * rand_vocab out of range with p_random > 0, whole_word without starts, labels aliasing ids or out)
 * or HIP error; -4 whole-word mode with a byte map holding an id >= 256 (lengths undefined, as for
 * spans); -6 bad row_off.  (A HIP error after the first piece of shred_mlm_rows leaves the earlier
 * pieces' output in place.)
 *
 * out may be the same buffer as ids (in place).  labels must not alias either.  p == 0 is legal: a
 * copy, all labels ignore_id, returns 0.
 *
 * The masking scratch (two result words, events, the host call's staging, and in whole-word mode 9 B
 * per id for the word begins and k') is allocated on the first masking call and freed with the
 * encoder, so the other calls' footprints are unchanged.  Whole-word mode reads the token-lengths
 * table of the span passes on the device and uploads it if no spans call has.
 */
#define SHRED_MLM_MAX_PROTECT 16

typedef struct ShredMlmOpts {
  uint64_t index_base;
  double p;
  uint64_t seed;
  double p_mask, p_random;
  int32_t mask_id;
  int32_t ignore_id;
  int64_t rand_vocab;
  const int32_t* protect;
  size_t protect_n;
  int protect_specials;
  int whole_word;
} ShredMlmOpts;

/* All buffers on the encoder's device (row_off is validated there, and a bad one keeps the later
 * passes from writing); queued on `stream` (NULL = the encoder's own) and synchronised before
 * return.  ids, out and labels need only their element's alignment, so tensor views fit.  kernel_ms
 * (may be NULL) receives the device time of the passes. */
int64_t shred_mlm_device(ShredEncoder* enc, const void* ids, size_t n, const void* row_off, size_t rows,
                         const ShredMlmOpts* opts, const void* starts, void* out, void* labels, void* stream,
                         double* kernel_ms);

/* Host buffers, staged through cached device buffers in pieces of whole rows under the piece budget
 * of the batch calls, so device memory does not grow with n (one row is taken whole, however long).
 * Each piece runs the device passes with index_base + the index of its first id; because words never
 * cross rows and positions are global, the result is the same for every piece size.  row_off is
 * validated on the host before anything is staged. */
int64_t shred_mlm_rows(ShredEncoder* enc, const int32_t* ids, size_t n, const int64_t* row_off, size_t rows,
                       const ShredMlmOpts* opts, const int64_t* starts, int32_t* out, int32_t* labels);

/* ---- span-corruption inputs and targets on the GPU (T5 / UL2 denoising) ----------------------------
 *
 * The encoder-decoder denoising objective (T5, UL2, ByT5, BART-style infilling) removes spans of
 * tokens from the input, leaves one sentinel where each was, and asks the decoder for the spans, each
 * behind its sentinel.  These calls work on the flat (ids, row_off) pair and return two flat streams
 * in the same format, the input and the target, so pad, pack, window and decode take both unchanged.
 *
 * Inputs:
 *   ids         n int32.
 *   row_off     the usual rows + 1 int64, or NULL with rows == 0 for one row; validated as elsewhere (-6).
 *   opts        the scalar options, ShredCorruptOpts below:
 *     index_base, seed   as in ShredMlmOpts.
 *     p_start            in [0, 1]: the probability that a position starts a span.
 *     len_cum, len_n     host pointer to 1 <= len_n <= SHRED_CORRUPT_MAX_SPAN uint64 values
 *                        C_1 <= ... <= C_len_n with C_len_n == 2^32; C_i = 2^32 * P(L <= i) for the
 *                        span length L.  Anything else returns -1.
 *     sentinel_first, sentinel_step, sentinel_n
 *                        sentinel j is S_j = sentinel_first + j * sentinel_step, computed in int32;
 *                        -1 when sentinel_n > 0 and S_{sentinel_n - 1} leaves int32, or sentinel_n < 0.
 *                        T5 uses (V - 1, -1, 100).
 *     final_sentinel     non-zero: every target row ends with the next unused sentinel (T5's closing one).
 *     protect, protect_n, protect_specials   as in ShredMlmOpts, with the same limit.
 *
 * Definitions.  mix, G, d(x, c) and T(q) are those of the masked-LM section; the constants are
 * START = (1 << 40) + 2 and LEN = (1 << 40) + 3, so one seed gives draws unrelated to dropout and masking.
 *   Position k, with h = index_base + k:
 *             starts a span iff (d(h, START) >> 32) < T(p_start), whatever its id;
 *             has the length L(k) = 1 + #{ i in [1, len_n) : v >= C_i }, v = d(h, LEN) >> 32;
 *             has the reach min(k + L(k), the end of k's row).
 *   Token j is noise iff it is not guarded (the protect list, and the specials under protect_specials)
 *             and some start k has k <= j < reach(k).  A reach never passes a row's end, so no span
 *             crosses rows; a guarded token inside a span stays in the input and splits it.
 *   A run is a maximal sequence of consecutive noise tokens of one row.  The runs of a row have the
 *             ranks 0, 1, ...  With Rmax = max(sentinel_n - (final_sentinel != 0), 0), the runs of
 *             rank >= Rmax are not corrupted: their tokens count as ordinary tokens from here on.
 *             J_r: the number of corrupted runs of row r.
 *   Input row r:   the row's tokens in order, every corrupted run replaced by its one sentinel S_rank.
 *   Target row r:  for every corrupted run in order, S_rank and then the run's tokens; with
 *             final_sentinel and sentinel_n > 0, S_{J_r} after them.  A row without noise (an empty
 *             one too) is then just [S_0].
 *
 * Outputs:
 *   in_ids, tgt_ids          in_cap and tgt_cap int32: the two streams.
 *   in_row_off, tgt_row_off  rows + 1 int64 each (2 without row_off), in the line_off format over
 *                            their own streams.
 *   in_src                   NULL, or in_cap int64: for every input id, the index in ids of a kept
 *                            token, or of its run's first token for a sentinel.  The same index into
 *                            the starts of shred_encode_spans / shred_encode_docs is its byte offset.
 *   *tgt_n                   (may be NULL) T_tgt, the number of target ids.
 *
 * Returns T_in, the number of input ids.  T_in <= n, because every token puts at most one id into
 * the input (itself, or its run's sentinel in the place of the run's first token).  T_tgt <= 2 n +
 * rows, because a token puts at most two ids into the target (a run of one token: its sentinel and
 * itself) and a row at most one closing sentinel.  So in_cap = n and tgt_cap = 2 n + rows (2 n + 1
 * without row_off) always suffice.  If in_ids or tgt_ids is NULL, or a cap is too small, nothing but
 * *tgt_n is written: the sizing call.
 *
 * Errors, with nothing written: -1 bad argument (above; p_start outside [0, 1] or NaN; protect_n above
 * the limit; in_ids and tgt_ids without both offset arrays; in_ids or tgt_ids aliasing ids) or HIP
 * error; -6 bad row_off.  (A HIP error after the first piece of shred_corrupt_rows leaves the earlier
 * pieces' output in place.)
 *
 * A decision depends on (seed, index_base + k, ids) alone: host and device calls, and every piece
 * size, agree, and a new seed (per epoch, say) gives a new corruption.
 *
 * The corruption scratch (three result words, events, 1 B per id and 48 B per 1024 ids of the largest
 * call, the scans' scratch and the host call's staging) is allocated on the first corrupt call and
 * freed with the encoder, so the other calls' footprints are unchanged.
 */
#define SHRED_CORRUPT_MAX_SPAN 32

typedef struct ShredCorruptOpts {
  uint64_t index_base;
  uint64_t seed;
  double p_start;
  const uint64_t* len_cum;
  size_t len_n;
  int32_t sentinel_first, sentinel_step, sentinel_n;
  int final_sentinel;
  const int32_t* protect;
  size_t protect_n;
  int protect_specials;
} ShredCorruptOpts;

/* All buffers on the encoder's device (row_off is validated there, and a bad one keeps the later
 * passes from writing); queued on `stream` (NULL = the encoder's own) and synchronised before
 * return.  Every buffer needs only its element's alignment, so tensor views fit.  kernel_ms (may be
 * NULL) receives the device time of the passes. */
int64_t shred_corrupt_device(ShredEncoder* enc, const void* ids, size_t n, const void* row_off, size_t rows,
                             const ShredCorruptOpts* opts, void* in_ids, size_t in_cap, void* in_row_off, void* in_src,
                             void* tgt_ids, size_t tgt_cap, void* tgt_row_off, size_t* tgt_n, void* stream,
                             double* kernel_ms);

/* Host buffers, staged through cached device buffers in pieces of whole rows under the piece budget
 * of the batch calls (one row is taken whole, however long).  Each piece runs the device passes with
 * index_base + the index of its first id; spans never cross rows and positions are global, so the
 * result is the same for every piece size.  row_off is validated on the host before anything is
 * staged.  Caps below n and 2 n + rows cost a round of counting passes before the writing one. */
int64_t shred_corrupt_rows(ShredEncoder* enc, const int32_t* ids, size_t n, const int64_t* row_off, size_t rows,
                           const ShredCorruptOpts* opts, int32_t* in_ids, size_t in_cap, int64_t* in_row_off,
                           int64_t* in_src, int32_t* tgt_ids, size_t tgt_cap, int64_t* tgt_row_off, size_t* tgt_n);

/* ---- fill-in-the-middle rows on the GPU (FIM) -------------------------------------------------------
 *
 * The infilling objective of decoder-only code models (Bavarian et al. 2022; SantaCoder, StarCoder, Code
 * Llama, DeepSeek-Coder) cuts a document into prefix, middle and suffix and re-emits them with three
 * sentinels, the middle last, so that an ordinary left-to-right model learns to fill it in.  These calls
 * work on the flat (ids, row_off) pair and return one flat stream in the same format, so pad, pack,
 * window and decode take it unchanged; bos / eos come from those calls as usual.
 *
 * Inputs:
 *   ids         n int32.
 *   row_off     the usual rows + 1 int64, or NULL with rows == 0 for one row; validated as elsewhere (-6).
 *               R below is the number of rows, 1 without row_off.
 *   opts        the scalar options, ShredFimOpts below:
 *     row_base           uint64 added to every row index below.  The host call's pieces use it; a caller
 *                        sharding a stream over calls may use it too.
 *     seed               a 64-bit seed.
 *     fim_rate, spm_rate in [0, 1]: the share of rows transformed, and of those the share in SPM order.
 *     min_len            >= 0: shorter rows are never transformed.
 *     pre_id, suf_id, mid_id   the three sentinels, any int32.  Callers pass registered specials' ids.
 *   cuts        NULL, or R x 3 int64 (a, b, mode) per row; the triple -1, -1, -1 means "not
 *               transformed".  When given, no draw is made and the rows are assembled by it (the
 *               character-level path below uses this).  Each triple must be all -1, or have
 *               0 <= a <= b <= L and mode in {0, 1}: anything else returns -8.
 *
 * Definitions.  mix, G, d(x, c) and T(q) are those of the masked-LM section; the constants are
 * FIM = (1 << 40) + 4, CUT_A = (1 << 40) + 5, CUT_B = (1 << 40) + 6 and MODE = (1 << 40) + 7, beside
 * START and LEN of span corruption.  Decisions are per row, not per token.  Row r of length L, with
 * h = row_base + r:
 *   is transformed iff L >= min_len and (d(h, FIM) >> 32) < T(fim_rate);
 *   has the cuts x = ((d(h, CUT_A) >> 32) * (L + 1)) >> 32 and y, the same from CUT_B (in uint64
 *             arithmetic), a = min(x, y), b = max(x, y), so 0 <= a <= b <= L: the prefix is [0, a), the
 *             middle [a, b) and the suffix [b, L) of the row;
 *   has the mode 1 (SPM) iff (d(h, MODE) >> 32) < T(spm_rate), else 0 (PSM).
 *   Output row, PSM:  pre_id, prefix, suf_id, suffix, mid_id, middle.
 *   Output row, SPM:  pre_id, suf_id, suffix, mid_id, prefix, middle (the Code Llama order).
 *             Its length is L + 3.  A row that is not transformed is copied, length L.  L == 0 is legal
 *             and gives the three sentinels when transformed.
 *
 * Outputs:
 *   out_ids      out_cap int32: the stream.
 *   out_row_off  R + 1 int64, in the line_off format over the stream.
 *   out_src      NULL, or out_cap int64: for every output id the index in ids of the token it copies,
 *                or -1 for a sentinel.  The same index into the starts of shred_encode_spans /
 *                shred_encode_docs is its byte offset.
 *   out_seg      NULL, or out_cap uint8, for a loss on the middle only: 0 = row not transformed,
 *                1 = prefix, 2 = suffix, 3 = middle, 4 = sentinel.
 *   row_info     NULL, or R x 3 int64 in the format of cuts: what was drawn or given.
 *
 * Returns T_out = n + 3 F, where F is the number of transformed rows; out_cap = n + 3 R always
 * suffices.  If out_ids is NULL or out_cap < T_out, nothing is written: the sizing call.
 *
 * Errors, with nothing written: -1 bad argument (a rate outside [0, 1] or NaN; min_len < 0; out_ids
 * without out_row_off; out_ids aliasing ids) or HIP error; -6 bad row_off; -8 bad cuts.  (A HIP error
 * after the first piece of shred_fim_rows leaves the earlier pieces' output in place.)
 *
 * A decision depends on (seed, row_base + r, L) alone: host and device calls, and every piece size,
 * agree, and a new seed (per epoch, say) gives a new transformation.
 *
 * The FIM scratch (three result words, events, 48 B per row of the largest call, the scan's scratch
 * and the host call's staging) is allocated on the first FIM call and freed with the encoder, so the
 * other calls' footprints are unchanged.
 */
typedef struct ShredFimOpts {
  uint64_t row_base;
  uint64_t seed;
  double fim_rate, spm_rate;
  int64_t min_len;
  int32_t pre_id, suf_id, mid_id;
} ShredFimOpts;

/* All buffers on the encoder's device (row_off and cuts are validated there, and a bad one keeps the
 * later passes from writing); queued on `stream` (NULL = the encoder's own) and synchronised before
 * return.  Every buffer needs only its element's alignment, so tensor views fit.  kernel_ms (may be
 * NULL) receives the device time of the passes. */
int64_t shred_fim_device(ShredEncoder* enc, const void* ids, size_t n, const void* row_off, size_t rows,
                         const ShredFimOpts* opts, const void* cuts, void* out_ids, size_t out_cap, void* out_row_off,
                         void* out_src, void* out_seg, void* row_info, void* stream, double* kernel_ms);

/* Host buffers, staged through cached device buffers in pieces of whole rows under the piece budget
 * of the batch calls (one row is taken whole, however long).  Each piece runs the device passes with
 * row_base + its first row and its slice of cuts, so the result is the same for every piece size.
 * row_off and cuts are validated on the host before anything is staged.  A cap below n + 3 R costs a
 * round of counting passes before the writing one. */
int64_t shred_fim_rows(ShredEncoder* enc, const int32_t* ids, size_t n, const int64_t* row_off, size_t rows,
                       const ShredFimOpts* opts, const int64_t* cuts, int32_t* out_ids, size_t out_cap,
                       int64_t* out_row_off, int64_t* out_src, uint8_t* out_seg, int64_t* row_info);

/* Character-level cuts: the FIM paper recommends cutting the text, not the tokens, so that the model
 * sees broken tokens at the joins.  text (n bytes) and doc_off (NULL with docs == 0: one document;
 * else docs + 1 int64, validated as in shred_encode_docs_device, -6) on the device.  Document d, bytes
 * [s, e) with B = e - s and h = row_base + d, takes the three draws above with L = B (min_len is in
 * bytes here).  Both cuts are then snapped to UTF-8.  snap(p): while p > 0, p < B,
 * (text[s + p] & 0xC0) == 0x80 and fewer than 3 steps have been taken, p -= 1.  a' = snap(a),
 * b' = max(snap(b), a').
 *   piece_off   3 * D + 1 int64 (D = docs, 1 without doc_off): s, s + a', s + b' for a transformed
 *               document and s, e, e for one that is not; the last entry is n.  It is a doc_off of
 *               3 D documents: shred_encode_docs_device encodes every piece as if alone.
 *   doc_mode    D int8: -1 not transformed, 0 PSM, 1 SPM.
 * With the row offsets R3 that shred_encode_docs_device returns for piece_off, document d is the row
 * [R3[3 d], R3[3 d + 3]) with cuts = (R3[3 d + 1] - R3[3 d], R3[3 d + 2] - R3[3 d], doc_mode[d]), or all
 * -1, for shred_fim_device.  A cut that falls inside a special token's bytes leaves ordinary text on
 * both sides.  Returns 0, -1 (bad argument, as above, or HIP error) or -6, with nothing written then.
 * A device-only entry point: both outputs on the device, queued and timed as above. */
int shred_fim_cuts_device(ShredEncoder* enc, const void* text, size_t n, const void* doc_off, size_t docs,
                          const ShredFimOpts* opts, void* piece_off, void* doc_mode, void* stream, double* kernel_ms);

/* Largest vocabulary (sum of all token byte lengths) the device decoder holds. */
#define SHRED_DECODE_MAX_VOCAB_BYTES (1u << 30)
/* Longest replacement for ids outside the vocabulary. */
#define SHRED_DECODE_MAX_UNK 8

#ifdef __cplusplus
}
#endif
#endif /* SHREDWORD_ENCODE_H */
