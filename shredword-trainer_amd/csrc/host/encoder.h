// Shared pieces of the BPE encoder (include/shredword_encode.h): the merge-rank table layout that
// the host builds and the gfx950 kernels probe, and the device half's interface.  No HIP type
// appears here so host C++ can include it; encode_device.hip implements EncodeDevice.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace shred {

// Open-addressing table, one u64 per slot: key (first << 20 | second, 40 bits) << 20 | rank.
// Capacity is a power of two >= 2 x merges (load factor <= 1/2); linear probing from
// enc_slot(key).  Ids outside [0, 2^20) never merge; an empty slot is all ones.
constexpr uint64_t kEncEmpty = ~0ull;
constexpr int32_t kEncIdLimit = 1 << 20;
constexpr int kEncMaxWord = 1024;  // SHRED_ENCODE_MAX_WORD

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

class EncodeDevice {
 public:
  // Uploads the table and byte map to `device`; *why says what failed.
  static EncodeDevice* create(int device, const std::vector<uint64_t>& table, const int32_t* byte_map,
                              std::string* why);
  ~EncodeDevice();
  // text / out on the device; stream = hipStream_t or nullptr.  Returns ids, -1 device error,
  // -2 cap too small, -3 word longer than kEncMaxWord.
  int64_t encode(const uint8_t* text, size_t n, int32_t* out, size_t cap, void* stream, double* kernel_ms);
  // Host buffers: staged through cached device buffers in pieces of <= kHostPiece bytes cut at
  // delimiters (device memory ~14 B per piece byte, whatever n is).
  static constexpr size_t kHostPiece = size_t(256) << 20;
  int64_t encode_host(const uint8_t* text, size_t n, int32_t* out, size_t cap);
  // Calls that fell back from the word cache to the direct path (overflow or hash collision).
  uint64_t fallbacks() const { return fallbacks_; }

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
  int64_t encode_special(const uint8_t* text, size_t n, int32_t* out, size_t cap, const std::vector<int32_t>& lens,
                         void* stream, double* enc_ms, double* special_ms);

  // ---- batches of documents (encode_docs.hip; include/shredword_encode.h defines the rows) ----
  // text (n bytes), doc_off (nullptr with docs == 0: one document; else docs + 1 entries, validated
  // on the device) and the outputs on the device: out (cap ids), starts (nullptr or cap int64; each
  // gets start_base added), row_off (rows + 1 int64).  specials: the ids come from encode_special().
  // kernel_ms: nullptr or 4 doubles (encode, span, special, document passes).  Returns as
  // encode_spans(), -6 for a bad doc_off.
  int64_t encode_docs(const uint8_t* text, size_t n, const int64_t* doc_off, size_t docs, bool specials, int32_t* out,
                      size_t cap, int64_t* starts, int64_t* row_off, uint64_t start_base,
                      const std::vector<int32_t>& lens, void* stream, double* kernel_ms);
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

 private:
  EncodeDevice() = default;
  bool reserve(size_t n, std::string* why);
  bool reserve_host(size_t n);
  // Span passes over n text bytes and their T ids (both on the device): starts[k] = start_base +
  // byte offset, line[q + 1] = id_base + id offset of the line after the q-th '\n' (line[0] is
  // not written; line_cap entries).  *newlines / *last_byte: the text's '\n' count and last byte.
  // Returns 0, -1 on a device error, -2 when line_cap < newlines + 1 (whole: < lines + 1, the
  // caller writes line[lines]); nothing is written then.
  int span_passes(const uint8_t* text, size_t n, const int32_t* ids, size_t T, int64_t* starts, int64_t* line,
                  size_t line_cap, uint64_t start_base, uint64_t id_base, bool whole,
                  const std::vector<int32_t>& lens, void* stream, size_t* newlines, uint8_t* last_byte, double* ms);
  bool reserve_spans(size_t n, size_t T, const std::vector<int32_t>& lens);
  void free_spans();  // called by the destructor
  int device_ = 0;
  void* stream_ = nullptr;      // hipStream_t
  uint64_t* table_ = nullptr;
  uint64_t mask_ = 0;
  bool packed_ = false;         // 16-bit LDS strips (ids < 0xFFFF)
  int32_t* byte_map_ = nullptr;
  // scratch sized for the largest text seen: ids per word span, rank cache of long words,
  // per-thread counts, per-block counts / offsets, total + error word
  size_t cap_bytes_ = 0;
  int32_t* pad_ = nullptr;
  int32_t* rank_ = nullptr;
  uint32_t* tcnt_ = nullptr;
  uint64_t* bcnt_ = nullptr;    // [0, nb) block counts, [nb, 2 nb) inclusive sums
  void* scan_tmp_ = nullptr;     // hipCUB scan scratch
  size_t scan_tmp_bytes_ = 0;
  uint64_t* misc_ = nullptr;    // [0] total ids, [1] flags: 1 long word, 2 probe window full, 4 collision,
                                // 8 arena full; [2] word-cache arena top
  // word cache (one 16-byte slot per distinct word): 64-bit word hash, payload (an occurrence's
  // offset, then arena offset | length << 32 | id count << 48); the arena is rank_
  size_t ccap_ = 0, ccap_min_ = 0;  // allocated slots; slots a call starts with
  uint64_t* cslot_ = nullptr;
  uint64_t* host_misc_ = nullptr;  // pinned
  // host-path staging
  size_t host_cap_ = 0;
  uint8_t* dtext_ = nullptr;
  int32_t* dout_ = nullptr;
  void* ev_[4] = {nullptr, nullptr, nullptr, nullptr};
  uint64_t fallbacks_ = 0;
  // span passes (encode_spans.hip): allocated on the first spans call, never by encode()
  int32_t* sp_lens_ = nullptr;     // 256 + M token lengths
  size_t sp_chunks_ = 0;           // chunks sp_cnt_ holds
  uint64_t* sp_cnt_ = nullptr;     // 4 x chunks: non-delimiter / '\n' counts, their inclusive sums
  size_t sp_ids_ = 0;              // ids sp_prefix_ holds
  uint64_t* sp_prefix_ = nullptr;  // P[k]: source bytes of the ids before k
  void* sp_tmp_ = nullptr;         // hipCUB scan scratch
  size_t sp_tmp_bytes_ = 0;
  uint64_t* sp_host_ = nullptr;    // pinned: '\n' total, last text byte
  void* sp_ev_[4] = {nullptr, nullptr, nullptr, nullptr};
  // host-path staging of the span outputs
  size_t sp_hstarts_cap_ = 0, sp_hline_cap_ = 0;
  int64_t* sp_hstarts_ = nullptr;
  int64_t* sp_hline_ = nullptr;

  // special passes (encode_special.hip): allocated on the first special call, never by the others
  bool reserve_special(size_t n);
  void free_special();  // called by the destructor
  std::vector<uint8_t> sx_bytes_;    // the registered specials' bytes, in id order
  std::vector<uint32_t> sx_off_;     // K + 1 offsets into sx_bytes_
  int32_t sx_first_id_ = 0;          // id of special 0
  bool sx_dirty_ = false;            // the device table is older than the set
  uint32_t* sx_tab_ = nullptr;       // scan table: first-byte set, groups, entries, bytes
  uint32_t sx_tab_words_ = 0, sx_tab_ent_ = 0, sx_tab_bytes_ = 0;  // its size, entry and byte word offsets
  size_t sx_cap_ = 0;                // text bytes the scratch below holds
  uint8_t* sx_text_ = nullptr;       // the text with the accepted matches blanked
  int32_t* sx_wids_ = nullptr;       // ids of the blanked text's words
  uint32_t* sx_cnt_ = nullptr;       // matches of the runs that start in each 32-byte span
  uint64_t* sx_inc_ = nullptr;       // their inclusive sum
  void* sx_tmp_ = nullptr;           // hipCUB scan scratch
  size_t sx_tmp_bytes_ = 0;
  size_t sx_ids_ = 0;                // entries sx_wstarts_ holds
  int64_t* sx_wstarts_ = nullptr;    // byte offsets of the word ids
  size_t sx_matches_ = 0;            // entries sx_mpos_ / sx_midx_ hold
  uint64_t* sx_mpos_ = nullptr;      // match positions, ascending
  uint32_t* sx_midx_ = nullptr;      // their specials
  uint64_t* sx_flag_ = nullptr;      // device: a run past kEncMaxWord
  uint64_t* sx_host_ = nullptr;      // pinned: match total, the flag
  void* sx_ev_[4] = {nullptr, nullptr, nullptr, nullptr};

  // document passes (encode_docs.hip): allocated on the first docs call, never by the others
  bool reserve_docs(size_t total);
  void free_docs();  // called by the destructor
  size_t dx_cap_ = 0;                // bytes dx_text_ holds
  uint8_t* dx_text_ = nullptr;       // the copy: every document followed by a '\n', none inside
  uint64_t* dx_flag_ = nullptr;      // device: bad doc_off
  uint64_t* dx_host_ = nullptr;      // pinned: the flag
  void* dx_ev_[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // around the check, the copy, the starts pass
  // host-path staging: a piece's document offsets, row offsets, starts (text and ids: dtext_ / dout_)
  size_t dx_hoff_cap_ = 0, dx_hrow_cap_ = 0, dx_hstarts_cap_ = 0;
  int64_t* dx_hoff_ = nullptr;
  int64_t* dx_hrow_ = nullptr;
  int64_t* dx_hstarts_ = nullptr;

  // decode passes (decode_device.hip): allocated on the first decode call, never by the encode calls
  struct DecodeCall;  // one call's arguments, as the kernels take them
  bool reserve_decode(size_t n, size_t rows, const std::vector<int32_t>& first, const std::vector<int32_t>& second);
  // Length passes over n device ids and their row_off (nullptr, or rows + 1 entries whose end
  // points are checked when c.ends): Q into dec_q_, *total = the bytes needed.  0, -1, -6.
  int decode_lengths(const DecodeCall& c, void* stream, uint64_t* total);
  // byte_off (nullptr, or as the header defines it, plus c.base) and the total bytes into out.
  int decode_expand(const DecodeCall& c, uint64_t total, uint8_t* out, int64_t* byte_off, void* stream);
  void free_decode();  // called by the destructor
  uint32_t dec_vocab_ = 0;           // 256 + M
  uint32_t* dec_tok_off_ = nullptr;  // 256 + M + 1 offsets into dec_arena_
  uint8_t* dec_arena_ = nullptr;     // the bytes of every token
  size_t dec_ids_ = 0;               // dec_q_ holds dec_ids_ + 1 entries
  uint64_t* dec_q_ = nullptr;        // Q[k]: output offset of token k; Q[n] = the total
  size_t dec_marks_ = 0;             // dec_mark_ holds dec_marks_ + 1 entries
  uint32_t* dec_mark_ = nullptr;     // rows that end just before id k (separators in front of it)
  void* dec_tmp_ = nullptr;          // hipCUB scan scratch
  size_t dec_tmp_bytes_ = 0;
  uint64_t* dec_err_ = nullptr;      // device: [0] an id outside the vocabulary, [1] bad row_off
  uint64_t* dec_host_ = nullptr;     // pinned: total, the two error words
  void* dec_ev_[4] = {nullptr, nullptr, nullptr, nullptr};
  // host-path staging: ids, row offsets, byte offsets, output bytes of a piece
  size_t dec_hids_cap_ = 0, dec_hrow_cap_ = 0, dec_hout_cap_ = 0;
  int32_t* dec_hids_ = nullptr;
  int64_t* dec_hrow_ = nullptr;      // 2 x dec_hrow_cap_: row offsets, then byte offsets
  uint8_t* dec_hout_ = nullptr;

  // batch passes (batch_device.hip): allocated on the first pad / pack call, never by the encode
  // or decode calls
  struct BatchCall;  // one call's (or piece's) rows, as the kernels take them
  bool reserve_batch(size_t rows);
  // Row checks (when c.row), E into bat_e_ (when scan) and max e_r over c's rows: 0, -1, -6.
  int batch_lengths(const BatchCall& c, bool scan, void* stream, uint64_t* total, uint64_t* widest);
  int pad_expand(const BatchCall& c, uint64_t width, int32_t pad_id, int pad_side, int32_t* out, int32_t* lengths,
                 uint8_t* mask, void* stream);
  // Stream positions [c.base, c.base + limit) into out / pos / seg (which point at position
  // c.base), pad_id from the rows' end on; row_start[r] = c.base + E[r] for the call's rows.
  int pack_expand(const BatchCall& c, uint64_t limit, int32_t pad_id, int32_t* out, int32_t* pos,
                  int32_t* seg, int64_t* row_start, void* stream);
  void free_batch();  // called by the destructor
  size_t bat_rows_ = 0;              // bat_e_ holds bat_rows_ + 1 entries
  uint64_t* bat_e_ = nullptr;        // E[r]: stream offset of emitted row r; E[rows] = T
  void* bat_tmp_ = nullptr;          // hipCUB scan / reduce scratch
  size_t bat_tmp_bytes_ = 0;
  uint64_t* bat_res_ = nullptr;      // device: [0] bad row_off, [1] an e_r past int32, [2] max e_r
  uint64_t* bat_host_ = nullptr;     // pinned: T, then the three words of bat_res_
  void* bat_ev_[4] = {nullptr, nullptr, nullptr, nullptr};
  // host-path staging: ids, row offsets, a piece's int32 outputs, its mask
  size_t bat_hids_cap_ = 0, bat_hrow_cap_ = 0, bat_hout_cap_ = 0, bat_hmask_cap_ = 0;
  int32_t* bat_hids_ = nullptr;
  int64_t* bat_hrow_ = nullptr;      // 2 x bat_hrow_cap_: row offsets, then row_start
  int32_t* bat_hout_ = nullptr;      // 3 x bat_hout_cap_: out, then pos / lengths, then seg
  uint8_t* bat_hmask_ = nullptr;
};

}  // namespace shred
