// Shared pieces of the BPE encoder (include/shredword_encode.h): the merge-rank table layout that
// the host builds and the gfx950 kernels probe, and the device half's interface.  No HIP type
// appears here so host C++ can include it; encode_device.hip implements EncodeDevice.
#pragma once

#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

namespace shred {

// Open-addressing table, one u64 per slot: key (first << 20 | second, 40 bits) << 20 | rank.
// Capacity is a power of two >= 2 x merges (load factor <= 1/2); linear probing from
// enc_slot(key).  Ids outside [0, 2^20) never merge; an empty slot is all ones.
constexpr uint64_t kEncEmpty = ~0ull;
constexpr int32_t kEncIdLimit = 1 << 20;
constexpr int kEncMaxWord = 1024;  // SHRED_ENCODE_MAX_WORD
constexpr uint32_t kEncMaxLongWord = 1u << 20;  // SHRED_ENCODE_MAX_LONG_WORD

inline uint64_t enc_key(int32_t a, int32_t b) { return (uint64_t)(uint32_t)a << 20 | (uint64_t)(uint32_t)b; }
inline uint64_t enc_slot(uint64_t key) { return (key * 0x9E3779B97F4A7C15ull) >> 24; }

// Builds the table; the first (lowest-rank) entry of a repeated pair wins, like the replay.
std::vector<uint64_t> enc_build_table(const std::vector<int32_t>& first, const std::vector<int32_t>& second);

// The decoder's vocabulary: off[i] .. off[i + 1] are the bytes of id i in `bytes` (256 + M ids; id
// 256 + m is first[m]'s bytes followed by second[m]'s).  False, with both left empty, when the
// bytes exceed kDecMaxVocabBytes.
constexpr uint64_t kDecMaxVocabBytes = 1ull << 30;  // SHRED_DECODE_MAX_VOCAB_BYTES
constexpr int kDecMaxUnk = 8;                       // SHRED_DECODE_MAX_UNK
bool enc_build_arena(const std::vector<int32_t>& first, const std::vector<int32_t>& second,
                     std::vector<uint32_t>* off, std::vector<uint8_t>* bytes);

// Windows of a row of len ids, C ids each and step ids apart (shred_window_*): the host's count and
// the kernels' (constexpr: usable in device code too).
constexpr uint64_t window_count(uint64_t len, uint64_t C, uint64_t step) {
  return len <= C ? 1 : 1 + (len - C + step - 1) / step;
}

// The batch calls (shred_pad_* .. shred_pair_*): "no limit" on the ids a row keeps, and the most
// rows a call takes (its row kernels run one workgroup per kBatchRowsPerGroup rows).
constexpr uint64_t kNoLimit = ~0ull;
constexpr uint64_t kBatchRowsPerGroup = 256;
constexpr bool batch_rows_fit(uint64_t rows) { return rows / kBatchRowsPerGroup < 0x7FFFFFFFull; }

// What one family of passes owns on the device; the units derive theirs from the resources of
// hip/encode_common.h.
struct PassState {
  virtual ~PassState() = default;
  virtual void specials_changed() {}  // set_specials(): drop what was built from the old set
};

class EncodeDevice {
 public:
  // Uploads the table and byte map to `device`; *why says what failed.
  static EncodeDevice* create(int device, const std::vector<uint64_t>& table, const int32_t* byte_map,
                              std::string* why);
  ~EncodeDevice();
  // text / out on the device; stream = hipStream_t or nullptr.  Returns ids, -1 device error,
  // -2 cap too small, -3 word longer than max_word().  pos_base: the position of text[0] in the text
  // passed to the C call (the host paths' pieces; only dropout looks at positions).
  int64_t encode(const uint8_t* text, size_t n, int32_t* out, size_t cap, void* stream, double* kernel_ms,
                 uint64_t pos_base = 0);
  // Host buffers: staged through cached device buffers in pieces of <= kHostPiece bytes cut at
  // delimiters (device memory ~14 B per piece byte, whatever n is).
  static constexpr size_t kHostPiece = size_t(256) << 20;
  int64_t encode_host(const uint8_t* text, size_t n, int32_t* out, size_t cap);
  // Calls that fell back from the word cache to the direct path (overflow or hash collision).
  uint64_t fallbacks() const { return fallbacks_; }

  // ---- words above kEncMaxWord (encode_long.hip; shred_encoder_set_long_words) ----
  // on: every encode call takes words of up to kEncMaxLongWord bytes; -3 then means a longer one.
  void set_long_words(bool on) { long_words_ = on; }
  bool long_words() const { return long_words_; }
  size_t max_word() const { return long_words_ ? (size_t)kEncMaxLongWord : (size_t)kEncMaxWord; }
  // What the long pass holds and has done: bytes of device scratch allocated for long words (0
  // until a call meets one), long words encoded, rounds run.
  void long_stats(uint64_t* scratch_bytes, uint64_t* words, uint64_t* rounds) const;

  // ---- BPE-dropout (encode_dropout.hip; shred_encoder_set_dropout defines it) ----
  // p in [0, 1] and the seed; false (nothing changes) for any other p.  With a threshold
  // T = (uint64_t)(p * 2^32) > 0 every encode call takes the direct dropout kernels.
  bool set_dropout(double p, uint64_t seed);
  double dropout_p() const { return drop_p_; }
  uint64_t dropout_seed() const { return drop_seed_; }

  // encode() plus the span passes (encode_spans.hip): starts (nullptr or cap int64) and line_off
  // (nullptr or line_cap int64) on the device, as include/shredword_encode.h defines them.
  // lens: the 256 + M source-byte lengths of the ids (host; uploaded on the first call).
  // kernel_ms: nullptr or 2 doubles (encode passes, span passes).  Returns as encode(); -2 also
  // when line_cap < lines + 1 (*num_lines is set, line_off untouched).
  // specials: the ids come from encode_special() instead of encode() (lens then holds the special
  // tokens' lengths too, and kernel_ms 3 doubles: the third is the special passes).
  int64_t encode_spans(const uint8_t* text, size_t n, int32_t* out, size_t cap, int64_t* starts, int64_t* line_off,
                       size_t line_cap, size_t* num_lines, const std::vector<int32_t>& lens, void* stream,
                       double* kernel_ms, bool specials = false);
  // The same on host buffers, in the pieces of encode_host.
  int64_t encode_spans_host(const uint8_t* text, size_t n, int32_t* out, size_t cap, int64_t* starts,
                            int64_t* line_off, size_t line_cap, size_t* num_lines, const std::vector<int32_t>& lens,
                            bool specials = false);

  // ---- special tokens (encode_special.hip; include/shredword_encode.h defines the matching) ----
  // Replaces the set: special i is bytes[off[i] .. off[i + 1]) and gets id first_id + i (the
  // caller has validated the set).  The scan table is rebuilt on the next special call, the span
  // length table and the decode vocabulary on the next call that uses them.
  void set_specials(const uint8_t* bytes, const size_t* off, size_t K, int32_t first_id);
  // encode() with the registered special tokens matched in the text: out receives the word ids
  // and the special ids in text order.  Returns as encode().  lens: as encode_spans takes it.
  // enc_ms / special_ms: nullptr or the device time of the encode passes / of the special passes.
  // pos_base: as encode takes it.
  int64_t encode_special(const uint8_t* text, size_t n, int32_t* out, size_t cap, const std::vector<int32_t>& lens,
                         void* stream, double* enc_ms, double* special_ms, uint64_t pos_base = 0);

  // ---- batches of documents (encode_docs.hip; include/shredword_encode.h defines the rows) ----
  // text (n bytes), doc_off (nullptr with docs == 0: one document; else docs + 1 entries, validated
  // on the device) and the outputs on the device: out (cap ids), starts (nullptr or cap int64; each
  // gets start_base added), row_off (rows + 1 int64).  specials: the ids come from encode_special().
  // kernel_ms: nullptr or 4 doubles (encode, span, special, document passes).  Returns as
  // encode_spans(), -6 for a bad doc_off.  pos_base: the position of the copy's first byte in the copy
  // of the whole text (doc_off[first] + first for a piece that begins with document `first`).
  int64_t encode_docs(const uint8_t* text, size_t n, const int64_t* doc_off, size_t docs, bool specials, int32_t* out,
                      size_t cap, int64_t* starts, int64_t* row_off, uint64_t start_base,
                      const std::vector<int32_t>& lens, void* stream, double* kernel_ms, uint64_t pos_base = 0);
  // The same on host buffers, in pieces of whole documents (doc_off is validated on the host).
  int64_t encode_docs_host(const uint8_t* text, size_t n, const int64_t* doc_off, size_t docs, bool specials,
                           int32_t* out, size_t cap, int64_t* starts, int64_t* row_off,
                           const std::vector<int32_t>& lens);

  // ---- ids to bytes (decode_device.hip; arguments and results as include/shredword_encode.h
  // defines them for shred_decode_device / shred_decode_rows).  first / second: the merge list,
  // from which the device vocabulary (with the registered special tokens behind the merges) is
  // built and uploaded on the first call, and again after set_specials().  The callers have
  // checked the arguments' ranges; decode_host's have also checked row_off, the ids (strict mode)
  // and cap on the host, so it returns the bytes written or -1.
  int64_t decode(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, uint8_t* out, size_t cap,
                 int64_t* byte_off, int sep, const uint8_t* unk, int unk_len, const std::vector<int32_t>& first,
                 const std::vector<int32_t>& second, void* stream, double* kernel_ms);
  static constexpr size_t kDecodePiece = size_t(1) << 25;  // ids per piece of decode_host
  int64_t decode_host(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, uint8_t* out,
                      int64_t* byte_off, int sep, const uint8_t* unk, int unk_len,
                      const std::vector<int32_t>& first, const std::vector<int32_t>& second);

  // ---- rows of ids to padded batches and packed sequences (batch_device.hip; arguments and
  // results as include/shredword_encode.h defines them for shred_pad_* / shred_pack_*).  The
  // callers have checked the arguments' ranges.  pad / pack take device buffers and return the
  // width needed / S, -1 or -6.  pad_host / pack_host take host buffers whose row_off, width, cap
  // and S * seq_len = out_len the caller has checked on the host; they return 0 or -1.
  struct BatchOpts {
    bool has_bos, has_eos;
    int32_t bos, eos;
    uint64_t max_len;  // 0: unlimited, else >= has_bos + has_eos
    int trunc_side;
  };
  int64_t pad(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const BatchOpts& o, size_t width,
              int32_t pad_id, int pad_side, int32_t* out, size_t cap, int32_t* lengths, uint8_t* mask, void* stream,
              double* kernel_ms);
  int64_t pack(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const BatchOpts& o, size_t seq_len,
               int32_t pad_id, bool drop_last, int32_t* out, size_t cap, int32_t* pos, int32_t* seg,
               int64_t* row_start, void* stream, double* kernel_ms);
  static constexpr size_t kBatchPiece = size_t(1) << 24;  // ids per piece of pad_host / pack_host
  int pad_host(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const BatchOpts& o, size_t width,
               int32_t pad_id, int pad_side, int32_t* out, int32_t* lengths, uint8_t* mask);
  int pack_host(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const BatchOpts& o,
                uint64_t out_len, int32_t pad_id, int32_t* out, int32_t* pos, int32_t* seg, int64_t* row_start);

  // ---- long rows cut into overlapping windows (batch_device.hip; shred_window_*).  o.max_len is C +
  // add with C >= 1, o.trunc_side 0, stride < C (the callers have checked).  window takes device
  // buffers and returns Wn, -1 or -6, with the longest window in *widest; window_host takes host
  // buffers whose row_off, width and cap the caller has checked on the host and returns 0 or -1.
  int64_t window(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const BatchOpts& o, size_t stride,
                 size_t width, int32_t pad_id, int pad_side, int32_t* out, size_t cap, int32_t* lengths, uint8_t* mask,
                 int32_t* win_row, int64_t* win_src, int64_t* row_win, size_t* widest, void* stream,
                 double* kernel_ms);
  int window_host(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const BatchOpts& o, size_t stride,
                  size_t width, int32_t pad_id, int pad_side, int32_t* out, int32_t* lengths, uint8_t* mask,
                  int32_t* win_row, int64_t* win_src, int64_t* row_win);

  // ---- row pairs to one model input (batch_pair.hip; shred_pair_*).  The callers have checked the
  // arguments' ranges: mid_n <= 2, strategy in 0 .. 3, max_len == 0 or >= the added ids; strategies
  // 0 .. 2 come with max_a == stride == 0, strategy 3 with 0 < max_len <= INT32_MAX.  pair takes
  // device buffers and returns Wn, -1, -6 or -7, with the longest emitted row in *widest; pair_host
  // takes host buffers whose row_a / row_b, fit (host/pair_rule.h), width and cap the caller has
  // checked on the host and returns 0 or -1.
  struct PairOpts {
    bool has_bos, has_eos;
    int32_t bos, eos, mid[2];
    uint32_t mid_n;
    uint64_t max_len;  // 0: unlimited
    int trunc_side, strategy;
    uint64_t max_a, stride;
  };
  int64_t pair(const int32_t* ids_a, size_t n_a, const int64_t* row_a, const int32_t* ids_b, size_t n_b,
               const int64_t* row_b, size_t rows, const PairOpts& o, size_t width, int32_t pad_id, int pad_side,
               int32_t* out, size_t cap, uint8_t* types, uint8_t* mask, int32_t* lengths, int32_t* win_row,
               int32_t* seg_len, int64_t* seg_src, int64_t* row_win, size_t* widest, void* stream, double* kernel_ms);
  int pair_host(const int32_t* ids_a, size_t n_a, const int64_t* row_a, const int32_t* ids_b, size_t n_b,
                const int64_t* row_b, size_t rows, const PairOpts& o, size_t width, int32_t pad_id, int pad_side,
                int32_t* out, uint8_t* types, uint8_t* mask, int32_t* lengths, int32_t* win_row, int32_t* seg_len,
                int64_t* seg_src, int64_t* row_win);

  // ---- masked-LM inputs (batch_mask.hip; shred_mlm_*).  The callers have checked the arguments'
  // ranges and turned the probabilities into thresholds.  mask takes device buffers (starts: nullptr
  // unless o.whole_word) and returns the selected count, -1 or -6; mask_host takes host buffers whose
  // row_off the caller has checked on the host and returns the selected count or -1.  lens: as
  // encode_spans takes it (whole-word mode reads the span passes' copy on the device).
  static constexpr int kMaskMaxProtect = 16;  // SHRED_MLM_MAX_PROTECT
  struct MaskOpts {
    uint64_t index_base, seed;
    uint64_t t_sel, t_mask, t_act;  // T(p), T(p_mask), T(p_mask) + T(p_random) <= 2^32
    uint64_t rand_vocab;
    int32_t mask_id, ignore_id;
    int32_t sp_lo, sp_hi;           // the registered specials are the ids [sp_lo, sp_hi)
    bool protect_specials, whole_word;
    uint32_t protect_n;
    int32_t protect[kMaskMaxProtect];
  };
  int64_t mask(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const MaskOpts& o,
               const int64_t* starts, const std::vector<int32_t>& lens, int32_t* out, int32_t* labels, void* stream,
               double* kernel_ms);
  int64_t mask_host(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const MaskOpts& o,
                    const int64_t* starts, const std::vector<int32_t>& lens, int32_t* out, int32_t* labels);

  // ---- span-corruption inputs and targets (batch_corrupt.hip; shred_corrupt_*).  The callers have
  // checked the arguments' ranges and turned p_start into a threshold.  corrupt takes device buffers
  // and returns T_in, -1 or -6, with T_tgt in *tgt_n; the outputs are written when in_ids and tgt_ids
  // are given and the caps suffice.  corrupt_host takes host buffers whose row_off the caller has
  // checked on the host and returns T_in or -1.
  static constexpr int kCorruptMaxSpan = 32;  // SHRED_CORRUPT_MAX_SPAN
  struct CorruptOpts {
    uint64_t index_base, seed;
    uint64_t t_start;                    // T(p_start)
    uint32_t len_n;
    uint64_t len_cum[kCorruptMaxSpan];   // C_1 .. C_len_n
    int32_t sent_first, sent_step;
    uint64_t rmax;                       // runs of rank >= rmax are kept
    bool closing;                        // every target row ends with a sentinel
    int32_t sp_lo, sp_hi;                // the registered specials are the ids [sp_lo, sp_hi)
    bool protect_specials;
    uint32_t protect_n;
    int32_t protect[kMaskMaxProtect];
  };
  int64_t corrupt(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const CorruptOpts& o,
                  int32_t* in_ids, size_t in_cap, int64_t* in_row_off, int64_t* in_src, int32_t* tgt_ids,
                  size_t tgt_cap, int64_t* tgt_row_off, size_t* tgt_n, void* stream, double* kernel_ms);
  int64_t corrupt_host(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const CorruptOpts& o,
                       int32_t* in_ids, size_t in_cap, int64_t* in_row_off, int64_t* in_src, int32_t* tgt_ids,
                       size_t tgt_cap, int64_t* tgt_row_off, size_t* tgt_n);

  // ---- fill-in-the-middle rows (batch_fim.hip; shred_fim_*).  The callers have checked the arguments'
  // ranges and turned the rates into thresholds.  fim takes device buffers (cuts: nullptr, or 3 int64
  // per row, validated on the device) and returns T_out, -1, -6 or -8; the outputs are written when
  // out_ids is given and out_cap suffices.  fim_host takes host buffers whose row_off and cuts the
  // caller has checked on the host and returns T_out or -1.  fim_cuts (shred_fim_cuts_device) takes
  // device buffers and returns 0, -1 or -6.
  struct FimOpts {
    uint64_t row_base, seed;
    uint64_t t_fim, t_spm;  // T(fim_rate), T(spm_rate)
    int64_t min_len;
    int32_t pre_id, suf_id, mid_id;
  };
  int64_t fim(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const FimOpts& o, const int64_t* cuts,
              int32_t* out_ids, size_t out_cap, int64_t* out_row_off, int64_t* out_src, uint8_t* out_seg,
              int64_t* row_info, void* stream, double* kernel_ms);
  int64_t fim_host(const int32_t* ids, size_t n, const int64_t* row_off, size_t rows, const FimOpts& o,
                   const int64_t* cuts, int32_t* out_ids, size_t out_cap, int64_t* out_row_off, int64_t* out_src,
                   uint8_t* out_seg, int64_t* row_info);
  int fim_cuts(const uint8_t* text, size_t n, const int64_t* doc_off, size_t docs, const FimOpts& o,
               int64_t* piece_off, int8_t* doc_mode, void* stream, double* kernel_ms);

 private:
  EncodeDevice() = default;
  // The token-length table of the span passes on the device (encode_spans.hip), uploaded when it is
  // not there (the first use, or after set_specials); nullptr when that fails.
  const int32_t* span_lens(const std::vector<int32_t>& lens);
  // Span passes over n text bytes and their T ids (both on the device): starts[k] = start_base +
  // byte offset, line[q + 1] = id_base + id offset of the line after the q-th '\n' (line[0] is
  // not written; line_cap entries).  *newlines / *last_byte: the text's '\n' count and last byte.
  // Returns 0, -1 on a device error, -2 when line_cap < newlines + 1 (whole: < lines + 1, the
  // caller writes line[lines]); nothing is written then.
  int span_passes(const uint8_t* text, size_t n, const int32_t* ids, size_t T, int64_t* starts, int64_t* line,
                  size_t line_cap, uint64_t start_base, uint64_t id_base, bool whole,
                  const std::vector<int32_t>& lens, void* stream, size_t* newlines, uint8_t* last_byte, double* ms);
  // The long pass of encode(): finds the words of text above kEncMaxWord bytes and encodes each with
  // one workgroup, its ids to pad + the word's offset (pad: pad_cap >= n int32), its id count to
  // (*cnt)[offset / 32] (device memory of the pass; nullptr entries' worth when there is no long
  // word).  Returns 0, -1 on a device error, -3 for a word above kEncMaxLongWord.
  int long_pass(const uint8_t* text, size_t n, const uint64_t* table, const int32_t* byte_map, int32_t* pad,
                size_t pad_cap, void* stream, const uint32_t** cnt);
  // The word pass of encode() under dropout: what k_encode_words does (ids packed per span in pad,
  // tcnt, bcnt, the long-word flag in misc[1]; rank: its scratch; pad and rank hold scratch_cap >= n
  // int32), with the candidates at positions pos_base + offset dropped.  Returns 0, -1 on an error.
  int dropout_words(const uint8_t* text, size_t n, const uint64_t* table, const int32_t* byte_map, int32_t* pad,
                    int32_t* rank, size_t scratch_cap, uint32_t* tcnt, uint64_t* bcnt, uint64_t* misc,
                    const uint32_t* lcnt, uint64_t pos_base, void* stream);
  int device_ = 0;
  void* stream_ = nullptr;  // hipStream_t
  uint64_t mask_ = 0;       // of the merge-rank table
  bool packed_ = false;     // 16-bit LDS strips (ids < 0xFFFF)
  uint64_t fallbacks_ = 0;
  bool long_words_ = false;  // words above kEncMaxWord go to the long pass
  double drop_p_ = 0;        // dropout as set; drop_thresh_ = (uint64_t)(drop_p_ * 2^32), 0 = off
  uint64_t drop_seed_ = 0, drop_thresh_ = 0;
  // The registered special tokens (set_specials); the units build their device tables from them.
  std::vector<uint8_t> sx_bytes_;  // the specials' bytes, in id order
  std::vector<uint32_t> sx_off_;   // K + 1 offsets into sx_bytes_
  int32_t sx_first_id_ = 0;        // id of special 0
  bool sx_dirty_ = false;          // the scan table on the device is older than the set
  // Everything a pass keeps on the device lives in its state, defined by the unit that runs the
  // pass and created on the pass's first call (kCore: by create()); the destructor destroys them.
  enum Pass { kCore, kStage, kSpans, kSpecial, kDocs, kDecode, kBatch, kWindow, kLong, kDropout, kPair, kMask,
              kCorrupt, kFim, kPasses };
  std::unique_ptr<PassState> pass_[kPasses];
};

}  // namespace shred
