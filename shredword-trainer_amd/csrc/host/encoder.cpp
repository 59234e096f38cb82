// C ABI of the BPE encoder (include/shredword_encode.h): reads the trainer's
// .model / .vocab files (written by reference bpe.cpp:388-432), validates the merge list, builds
// the merge-rank table and the byte map, and hands the text to the gfx950 kernels
// (encode_device.hip).  There is no host encoder: without a device the calls fail.
#include "shredword_encode.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "encoder.h"
#include "pair_rule.h"

namespace shred {

std::vector<uint64_t> enc_build_table(const std::vector<int32_t>& first, const std::vector<int32_t>& second) {
  size_t cap = 1024;
  while (cap < 2 * first.size()) cap <<= 1;
  std::vector<uint64_t> tab(cap, kEncEmpty);
  const uint64_t mask = cap - 1;
  for (size_t m = 0; m < first.size(); ++m) {
    const uint64_t key = enc_key(first[m], second[m]);
    for (uint64_t i = enc_slot(key) & mask;; i = (i + 1) & mask) {
      if (tab[i] == kEncEmpty) {
        tab[i] = key << 20 | (uint64_t)m;
        break;
      }
      if ((tab[i] >> 20) == key) break;  // a repeated pair: the lowest rank already holds it
    }
  }
  return tab;
}

bool enc_build_arena(const std::vector<int32_t>& first, const std::vector<int32_t>& second,
                     std::vector<uint32_t>* off, std::vector<uint8_t>* bytes) {
  const size_t M = first.size(), V = 256 + M;
  off->clear();
  bytes->clear();
  std::vector<uint64_t> o(V + 1);
  for (size_t i = 0; i <= 256; ++i) o[i] = i;
  for (size_t m = 0; m < M; ++m) {
    const size_t a = (size_t)first[m], b = (size_t)second[m];  // ids below 256 + m (split_merges)
    o[256 + m + 1] = o[256 + m] + (o[a + 1] - o[a]) + (o[b + 1] - o[b]);
    if (o[256 + m + 1] > kDecMaxVocabBytes) return false;
  }
  off->assign(o.begin(), o.end());
  bytes->resize((size_t)o[V]);
  for (size_t i = 0; i < 256; ++i) (*bytes)[i] = (uint8_t)i;
  for (size_t m = 0; m < M; ++m) {
    const size_t a = (size_t)first[m], b = (size_t)second[m];
    uint8_t* dst = bytes->data() + o[256 + m];
    std::memcpy(dst, bytes->data() + o[a], (size_t)(o[a + 1] - o[a]));
    std::memcpy(dst + (o[a + 1] - o[a]), bytes->data() + o[b], (size_t)(o[b + 1] - o[b]));
  }
  return true;
}

}  // namespace shred

struct ShredEncoder {
  std::vector<int32_t> first, second;
  int32_t byte_map[256];
  std::vector<std::string> tokens;  // bytes of every id (256 + merges + specials)
  std::vector<int32_t> lens;        // source bytes of every id, from the merge list and the specials alone
  size_t num_specials = 0;
  bool spans_ok = true;             // no byte maps to an id >= 256
  uint64_t vocab_bytes = 0;         // bytes of all tokens (the device decoder's arena)
  std::unique_ptr<shred::EncodeDevice> dev;
};

namespace {

bool read_file(const char* path, std::string* out) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  char buf[1 << 16];
  size_t r;
  out->clear();
  while ((r = std::fread(buf, 1, sizeof buf, f)) > 0) out->append(buf, r);
  std::fclose(f);
  return true;
}

ShredEncoder* make(std::vector<int32_t> first, std::vector<int32_t> second, const int32_t* byte_map, int device) {
  const size_t M = first.size();
  if (M + 256 > (size_t)shred::kEncIdLimit) {
    std::fprintf(stderr, "[ERROR]\t encoder: %zu merges exceed the id limit 2^20\n", M);
    return nullptr;
  }
  std::unique_ptr<ShredEncoder> e(new ShredEncoder());
  for (int b = 0; b < 256; ++b) e->byte_map[b] = byte_map ? byte_map[b] : b;
  e->tokens.resize(256 + M);
  for (int b = 0; b < 256; ++b) e->tokens[b] = std::string(1, (char)b);
  for (size_t m = 0; m < M; ++m) e->tokens[256 + m] = e->tokens[first[m]] + e->tokens[second[m]];
  e->lens.assign(256 + M, 1);
  for (size_t m = 0; m < M; ++m)
    e->lens[256 + m] = (int32_t)std::min<int64_t>((int64_t)e->lens[first[m]] + e->lens[second[m]], INT32_MAX);
  for (int b = 0; b < 256; ++b) e->spans_ok = e->spans_ok && e->byte_map[b] < 256;
  for (const std::string& t : e->tokens) e->vocab_bytes += t.size();
  std::string why;
  e->dev.reset(shred::EncodeDevice::create(device, shred::enc_build_table(first, second), e->byte_map, &why));
  if (!e->dev) {
    std::fprintf(stderr, "[ERROR]\t encoder: %s\n", why.c_str());
    return nullptr;
  }
  e->first = std::move(first);
  e->second = std::move(second);
  return e.release();
}

bool split_merges(const int32_t* triples, size_t M, std::vector<int32_t>* first, std::vector<int32_t>* second) {
  first->resize(M);
  second->resize(M);
  for (size_t m = 0; m < M; ++m) {
    const int32_t a = triples[3 * m], b = triples[3 * m + 1], id = triples[3 * m + 2];
    if (id != (int32_t)(256 + m) || a < 0 || b < 0 || a >= id || b >= id) {
      std::fprintf(stderr, "[ERROR]\t encoder: merge %zu (%d, %d -> %d) is not a trainer merge\n", m, a, b, id);
      return false;
    }
    (*first)[m] = a;
    (*second)[m] = b;
  }
  return true;
}

// Frequency column of a .vocab file: record i is "<token i without NUL bytes> <freq>\n" (the
// reference prints C strings, bpe.cpp:394-417).  False when the file does not match the tokens.
bool vocab_freqs(const std::string& v, const std::vector<std::string>& tokens, std::vector<uint64_t>* freq) {
  size_t pos = 0;
  freq->assign(tokens.size(), 0);
  for (size_t i = 0; i < tokens.size(); ++i) {
    for (char c : tokens[i]) {
      if (c == 0) continue;
      if (pos >= v.size() || v[pos] != c) return false;
      ++pos;
    }
    if (pos >= v.size() || v[pos] != ' ') return false;
    ++pos;
    uint64_t f = 0;
    size_t digits = 0;
    while (pos < v.size() && v[pos] >= '0' && v[pos] <= '9') f = f * 10 + (uint64_t)(v[pos++] - '0'), ++digits;
    if (!digits || pos >= v.size() || v[pos] != '\n') return false;
    ++pos;
    (*freq)[i] = f;
  }
  return pos == v.size();
}

}  // namespace

extern "C" {

ShredEncoder* shred_encoder_create(const int32_t* merges, size_t num_merges, const int32_t* byte_map, int device) {
  if (!merges && num_merges) return nullptr;
  std::vector<int32_t> first, second;
  if (!split_merges(merges, num_merges, &first, &second)) return nullptr;
  return make(std::move(first), std::move(second), byte_map, device);
}

ShredEncoder* shred_encoder_load(const char* model_path, const char* vocab_path, int32_t unk_id, int device) {
  if (!model_path) return nullptr;
  std::string model;
  if (!read_file(model_path, &model)) {
    std::fprintf(stderr, "[ERROR]\t encoder: couldn't open %s\n", model_path);
    return nullptr;
  }
  if (model.size() % 12) {
    std::fprintf(stderr, "[ERROR]\t encoder: %s is not a sequence of int32 triples\n", model_path);
    return nullptr;
  }
  const size_t M = model.size() / 12;
  std::vector<int32_t> triples(3 * M);
  if (M) std::memcpy(triples.data(), model.data(), model.size());
  std::vector<int32_t> first, second;
  if (!split_merges(triples.data(), M, &first, &second)) return nullptr;
  int32_t map[256];
  for (int b = 0; b < 256; ++b) map[b] = b;
  if (vocab_path) {
    std::string vocab;
    if (!read_file(vocab_path, &vocab)) {
      std::fprintf(stderr, "[ERROR]\t encoder: couldn't open %s\n", vocab_path);
      return nullptr;
    }
    std::vector<std::string> tokens(256 + M);
    for (int b = 0; b < 256; ++b) tokens[b] = std::string(1, (char)b);
    for (size_t m = 0; m < M; ++m) tokens[256 + m] = tokens[first[m]] + tokens[second[m]];
    std::vector<uint64_t> freq;
    if (!vocab_freqs(vocab, tokens, &freq)) {
      std::fprintf(stderr, "[ERROR]\t encoder: %s does not match the merges of %s\n", vocab_path, model_path);
      return nullptr;
    }
    // a byte the coverage rule dropped never has a symbol of its own and never merges
    bool used[256] = {false};
    for (size_t m = 0; m < M; ++m) {
      if (first[m] < 256) used[first[m]] = true;
      if (second[m] < 256) used[second[m]] = true;
    }
    for (int b = 0; b < 256; ++b)
      if (freq[b] == 0 && !used[b]) map[b] = unk_id;
  }
  return make(std::move(first), std::move(second), map, device);
}

void shred_encoder_destroy(ShredEncoder* enc) { delete enc; }

int shred_encoder_info(const ShredEncoder* enc, size_t* num_merges, int32_t* byte_map) {
  if (!enc) return -1;
  if (num_merges) *num_merges = enc->first.size();
  if (byte_map) std::memcpy(byte_map, enc->byte_map, sizeof enc->byte_map);
  return 0;
}

int shred_encoder_set_long_words(ShredEncoder* enc, int on) {
  if (!enc) return -1;
  enc->dev->set_long_words(on != 0);
  return 0;
}

int shred_encoder_long_words(const ShredEncoder* enc) { return enc && enc->dev->long_words() ? 1 : 0; }

int shred_encoder_long_stats(const ShredEncoder* enc, uint64_t* scratch_bytes, uint64_t* words, uint64_t* rounds) {
  if (!enc) return -1;
  enc->dev->long_stats(scratch_bytes, words, rounds);
  return 0;
}

int shred_encoder_set_dropout(ShredEncoder* enc, double p, uint64_t seed) {
  return enc && enc->dev->set_dropout(p, seed) ? 0 : -1;
}

int shred_encoder_dropout(const ShredEncoder* enc, double* p, uint64_t* seed) {
  if (!enc) return -1;
  if (p) *p = enc->dev->dropout_p();
  if (seed) *seed = enc->dev->dropout_seed();
  return 0;
}

int64_t shred_encode(ShredEncoder* enc, const uint8_t* text, size_t n, int32_t* out, size_t cap) {
  if (!enc || (n && (!text || !out))) return -1;
  return enc->dev->encode_host(text, n, out, cap);
}

int64_t shred_encode_device(ShredEncoder* enc, const void* text, size_t n, void* out, size_t cap, void* stream,
                            double* kernel_ms) {
  if (!enc || (n && (!text || !out))) return -1;
  return enc->dev->encode((const uint8_t*)text, n, (int32_t*)out, cap, stream, kernel_ms);
}

int shred_encoder_token_lengths(const ShredEncoder* enc, int32_t* out, size_t cap) {
  if (!enc || !out || cap < enc->lens.size()) return -1;
  std::memcpy(out, enc->lens.data(), enc->lens.size() * sizeof(int32_t));
  return 0;
}

int64_t shred_encode_spans(ShredEncoder* enc, const uint8_t* text, size_t n, int32_t* out, size_t cap,
                           int64_t* starts, int64_t* line_off, size_t line_cap, size_t* num_lines) {
  if (!enc || (n && (!text || !out))) return -1;
  if (!enc->spans_ok) return -4;
  return enc->dev->encode_spans_host(text, n, out, cap, starts, line_off, line_cap, num_lines, enc->lens);
}

int64_t shred_encode_spans_device(ShredEncoder* enc, const void* text, size_t n, void* out, size_t cap, void* starts,
                                  void* line_off, size_t line_cap, size_t* num_lines, void* stream,
                                  double* kernel_ms) {
  if (!enc || (n && (!text || !out))) return -1;
  if (!enc->spans_ok) return -4;
  return enc->dev->encode_spans((const uint8_t*)text, n, (int32_t*)out, cap, (int64_t*)starts, (int64_t*)line_off,
                                line_cap, num_lines, enc->lens, stream, kernel_ms);
}

int shred_encoder_set_specials(ShredEncoder* enc, const uint8_t* bytes, const size_t* offsets, size_t K) {
  if (!enc || K > SHRED_SPECIAL_MAX || (K && (!bytes || !offsets))) return -1;
  std::vector<std::string> sp(K);
  for (size_t i = 0; i < K; ++i) {
    if (offsets[i + 1] <= offsets[i] || offsets[i + 1] - offsets[i] > SHRED_SPECIAL_MAX_LEN) return -1;
    sp[i].assign((const char*)bytes + offsets[i], offsets[i + 1] - offsets[i]);
    if (sp[i].find_first_of("\t\r\n ") != std::string::npos) return -1;
    if (std::find(sp.begin(), sp.begin() + i, sp[i]) != sp.begin() + i) return -1;
  }
  const size_t V = 256 + enc->first.size();
  enc->tokens.resize(V);
  enc->lens.resize(V);
  for (const std::string& t : sp) {
    enc->tokens.push_back(t);
    enc->lens.push_back((int32_t)t.size());
  }
  enc->vocab_bytes = 0;
  for (const std::string& t : enc->tokens) enc->vocab_bytes += t.size();
  enc->num_specials = K;
  // (positions relative to the set's first byte: the device keeps its own copy)
  std::vector<size_t> off(K + 1, 0);
  for (size_t i = 0; i < K; ++i) off[i + 1] = off[i] + sp[i].size();
  enc->dev->set_specials(K ? bytes + offsets[0] : nullptr, off.data(), K, (int32_t)V);
  return 0;
}

size_t shred_encoder_num_specials(const ShredEncoder* enc) { return enc ? enc->num_specials : 0; }

int64_t shred_encode_special(ShredEncoder* enc, const uint8_t* text, size_t n, int32_t* out, size_t cap,
                             int64_t* starts, int64_t* line_off, size_t line_cap, size_t* num_lines) {
  if (!enc || (n && (!text || !out))) return -1;
  if (!enc->spans_ok) return -4;
  return enc->dev->encode_spans_host(text, n, out, cap, starts, line_off, line_cap, num_lines, enc->lens,
                                     enc->num_specials != 0);
}

int64_t shred_encode_special_device(ShredEncoder* enc, const void* text, size_t n, void* out, size_t cap,
                                    void* starts, void* line_off, size_t line_cap, size_t* num_lines, void* stream,
                                    double* kernel_ms) {
  if (kernel_ms) kernel_ms[2] = 0;
  if (!enc || (n && (!text || !out))) return -1;
  if (!enc->spans_ok) return -4;
  return enc->dev->encode_spans((const uint8_t*)text, n, (int32_t*)out, cap, (int64_t*)starts, (int64_t*)line_off,
                                line_cap, num_lines, enc->lens, stream, kernel_ms, enc->num_specials != 0);
}

int64_t shred_encode_docs(ShredEncoder* enc, const uint8_t* text, size_t n, const int64_t* doc_off, size_t docs,
                          int specials, int32_t* out, size_t cap, int64_t* starts, int64_t* row_off) {
  if (!enc || !row_off || (n && (!text || !out)) || (!doc_off && docs)) return -1;
  if (!enc->spans_ok) return -4;
  return enc->dev->encode_docs_host(text, n, doc_off, docs, specials != 0 && enc->num_specials != 0, out, cap, starts,
                                    row_off, enc->lens);
}

int64_t shred_encode_docs_device(ShredEncoder* enc, const void* text, size_t n, const void* doc_off, size_t docs,
                                 int specials, void* out, size_t cap, void* starts, void* row_off, void* stream,
                                 double* kernel_ms) {
  if (kernel_ms) kernel_ms[0] = kernel_ms[1] = kernel_ms[2] = kernel_ms[3] = 0;
  if (!enc || !row_off || (n && (!text || !out)) || (!doc_off && docs)) return -1;
  if (!enc->spans_ok) return -4;
  return enc->dev->encode_docs((const uint8_t*)text, n, (const int64_t*)doc_off, docs,
                               specials != 0 && enc->num_specials != 0, (int32_t*)out, cap, (int64_t*)starts,
                               (int64_t*)row_off, 0, enc->lens, stream, kernel_ms);
}

int64_t shred_decode(const ShredEncoder* enc, const int32_t* ids, size_t n, uint8_t* out, size_t cap) {
  if (!enc || (n && !ids)) return -1;
  size_t need = 0;
  for (size_t i = 0; i < n; ++i) {
    if (ids[i] < 0 || (size_t)ids[i] >= enc->tokens.size()) return -1;
    const std::string& t = enc->tokens[ids[i]];
    if (out && need + t.size() <= cap) std::memcpy(out + need, t.data(), t.size());
    need += t.size();
  }
  return (int64_t)need;
}

namespace {
// What both row decoders refuse before any work: 0, -1 or -5.
int decode_args(const ShredEncoder* enc, const void* ids, size_t n, const void* row_off, size_t rows, int sep,
                const uint8_t* unk, int unk_len) {
  if (!enc || (n && !ids) || (!row_off && rows) || sep < -1 || sep > 255) return -1;
  if (unk_len < -1 || unk_len > SHRED_DECODE_MAX_UNK || (unk_len > 0 && !unk)) return -1;
  if (enc->vocab_bytes > SHRED_DECODE_MAX_VOCAB_BYTES) return -5;
  return 0;
}
}  // namespace

int64_t shred_decode_device(ShredEncoder* enc, const void* ids, size_t n, const void* row_off, size_t rows,
                            void* out, size_t cap, void* byte_off, int sep, const uint8_t* unk, int unk_len,
                            void* stream, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0;
  if (const int r = decode_args(enc, ids, n, row_off, rows, sep, unk, unk_len)) return r;
  return enc->dev->decode((const int32_t*)ids, n, (const int64_t*)row_off, rows, (uint8_t*)out, cap,
                          (int64_t*)byte_off, sep, unk, unk_len, enc->first, enc->second, stream, kernel_ms);
}

int64_t shred_decode_rows(ShredEncoder* enc, const int32_t* ids, size_t n, const int64_t* row_off, size_t rows,
                          uint8_t* out, size_t cap, int64_t* byte_off, int sep, const uint8_t* unk, int unk_len) {
  if (const int r = decode_args(enc, ids, n, row_off, rows, sep, unk, unk_len)) return r;
  if (row_off) {
    if (row_off[0] != 0 || row_off[rows] < 0 || (uint64_t)row_off[rows] != n) return -6;
    for (size_t r = 0; r < rows; ++r)
      if (row_off[r] > row_off[r + 1]) return -6;
  }
  // the length pass of host ids: the sizing call and the capacity check need no device
  uint64_t need = sep >= 0 ? (row_off ? rows : 1) : 0;
  for (size_t i = 0; i < n; ++i) {
    if (ids[i] >= 0 && (size_t)ids[i] < enc->tokens.size()) need += enc->tokens[ids[i]].size();
    else if (unk_len < 0) return -1;
    else need += (uint64_t)unk_len;
  }
  if (!out || cap < need) return (int64_t)need;
  const int64_t r = enc->dev->decode_host(ids, n, row_off, rows, out, byte_off, sep, unk, unk_len, enc->first,
                                          enc->second);
  return r < 0 ? r : (int64_t)need;
}

namespace {
// What the four batch calls refuse before any work (0 or -1), and their options.
int batch_args(const ShredEncoder* enc, const void* ids, size_t n, const void* row_off, size_t rows,
               const int32_t* bos, const int32_t* eos, size_t max_len, int trunc_side,
               shred::EncodeDevice::BatchOpts* o) {
  if (!enc || (n && !ids) || (!row_off && rows) || trunc_side < 0 || trunc_side > 1) return -1;
  const size_t add = (bos ? 1 : 0) + (eos ? 1 : 0);
  if (max_len && max_len < add) return -1;
  *o = shred::EncodeDevice::BatchOpts{bos != nullptr, eos != nullptr, bos ? *bos : 0, eos ? *eos : 0,
                                      (uint64_t)max_len, trunc_side};
  return 0;
}

// An offset array of host rows: rows + 1 entries that start at 0, end at n and do not decrease.
bool offsets_ok(const int64_t* row_off, size_t rows, size_t n) {
  if (row_off[0] != 0 || row_off[rows] < 0 || (uint64_t)row_off[rows] != n) return false;
  for (size_t r = 0; r < rows; ++r)
    if (row_off[r] > row_off[r + 1]) return false;
  return true;
}

// The length pass of host rows: 0 with T = sum e_r and the largest e_r, -6 for a bad row_off, -1
// for an e_r past int32.
int batch_host_lengths(size_t n, const int64_t* row_off, size_t rows, const shred::EncodeDevice::BatchOpts& o,
                       uint64_t* total, uint64_t* widest) {
  const uint64_t add = (o.has_bos ? 1 : 0) + (o.has_eos ? 1 : 0);
  const uint64_t keep_max = o.max_len ? o.max_len - add : shred::kNoLimit;
  *total = *widest = 0;
  if (row_off && !offsets_ok(row_off, rows, n)) return -6;
  const size_t R = row_off ? rows : 1;
  for (size_t r = 0; r < R; ++r) {
    const uint64_t len = row_off ? (uint64_t)(row_off[r + 1] - row_off[r]) : (uint64_t)n;
    const uint64_t e = add + std::min(len, keep_max);
    if (e > (uint64_t)INT32_MAX) return -1;
    *total += e;
    *widest = std::max(*widest, e);
  }
  return 0;
}
}  // namespace

int64_t shred_pad_device(ShredEncoder* enc, const void* ids, size_t n, const void* row_off, size_t rows,
                         const int32_t* bos, const int32_t* eos, size_t max_len, int trunc_side, size_t width,
                         int32_t pad_id, int pad_side, void* out, size_t cap, void* lengths, void* mask,
                         void* stream, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0;
  shred::EncodeDevice::BatchOpts o;
  if (batch_args(enc, ids, n, row_off, rows, bos, eos, max_len, trunc_side, &o) || pad_side < 0 || pad_side > 1)
    return -1;
  return enc->dev->pad((const int32_t*)ids, n, (const int64_t*)row_off, rows, o, width, pad_id, pad_side,
                       (int32_t*)out, cap, (int32_t*)lengths, (uint8_t*)mask, stream, kernel_ms);
}

int64_t shred_pack_device(ShredEncoder* enc, const void* ids, size_t n, const void* row_off, size_t rows,
                          const int32_t* bos, const int32_t* eos, size_t max_len, int trunc_side, size_t seq_len,
                          int32_t pad_id, int drop_last, void* out, size_t cap, void* pos, void* seg,
                          void* row_start, void* stream, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0;
  shred::EncodeDevice::BatchOpts o;
  if (batch_args(enc, ids, n, row_off, rows, bos, eos, max_len, trunc_side, &o) || seq_len < 1 ||
      rows > (size_t)INT32_MAX)
    return -1;
  return enc->dev->pack((const int32_t*)ids, n, (const int64_t*)row_off, rows, o, seq_len, pad_id, drop_last != 0,
                        (int32_t*)out, cap, (int32_t*)pos, (int32_t*)seg, (int64_t*)row_start, stream, kernel_ms);
}

int64_t shred_pad_rows(ShredEncoder* enc, const int32_t* ids, size_t n, const int64_t* row_off, size_t rows,
                       const int32_t* bos, const int32_t* eos, size_t max_len, int trunc_side, size_t width,
                       int32_t pad_id, int pad_side, int32_t* out, size_t cap, int32_t* lengths, uint8_t* mask) {
  shred::EncodeDevice::BatchOpts o;
  if (batch_args(enc, ids, n, row_off, rows, bos, eos, max_len, trunc_side, &o) || pad_side < 0 || pad_side > 1)
    return -1;
  uint64_t total = 0, widest = 0;
  if (const int r = batch_host_lengths(n, row_off, rows, o, &total, &widest)) return r;
  const uint64_t R = row_off ? rows : 1;
  if (width && R > (uint64_t)INT64_MAX / width) return -1;
  if (!out || width < widest || cap < R * width) return (int64_t)widest;
  const int r = enc->dev->pad_host(ids, n, row_off, rows, o, width, pad_id, pad_side, out, lengths, mask);
  return r < 0 ? r : (int64_t)widest;
}

int64_t shred_pack_rows(ShredEncoder* enc, const int32_t* ids, size_t n, const int64_t* row_off, size_t rows,
                        const int32_t* bos, const int32_t* eos, size_t max_len, int trunc_side, size_t seq_len,
                        int32_t pad_id, int drop_last, int32_t* out, size_t cap, int32_t* pos, int32_t* seg,
                        int64_t* row_start) {
  shred::EncodeDevice::BatchOpts o;
  if (batch_args(enc, ids, n, row_off, rows, bos, eos, max_len, trunc_side, &o) || seq_len < 1 ||
      rows > (size_t)INT32_MAX)
    return -1;
  uint64_t total = 0, widest = 0;
  if (const int r = batch_host_lengths(n, row_off, rows, o, &total, &widest)) return r;
  const uint64_t L = seq_len;
  const uint64_t S = drop_last ? total / L : total / L + (total % L ? 1 : 0);
  if (S > (uint64_t)INT64_MAX / L) return -1;
  if (!out || cap < S * L) return (int64_t)S;
  const int r = enc->dev->pack_host(ids, n, row_off, rows, o, S * L, pad_id, out, pos, seg, row_start);
  return r < 0 ? r : (int64_t)S;
}

namespace {
// What the two window calls refuse before any work (0 or -1), and their options.
int window_args(const ShredEncoder* enc, const void* ids, size_t n, const void* row_off, size_t rows,
                const int32_t* bos, const int32_t* eos, size_t max_len, size_t stride, int pad_side,
                const void* win_row, shred::EncodeDevice::BatchOpts* o) {
  if (batch_args(enc, ids, n, row_off, rows, bos, eos, max_len, 0, o) || pad_side < 0 || pad_side > 1) return -1;
  const size_t add = (bos ? 1 : 0) + (eos ? 1 : 0);
  if (max_len <= add || max_len > (size_t)INT32_MAX || stride >= max_len - add) return -1;
  if (win_row && rows > (size_t)INT32_MAX) return -1;
  return 0;
}
}  // namespace

int64_t shred_window_device(ShredEncoder* enc, const void* ids, size_t n, const void* row_off, size_t rows,
                            const int32_t* bos, const int32_t* eos, size_t max_len, size_t stride, size_t width,
                            int32_t pad_id, int pad_side, void* out, size_t cap, void* lengths, void* mask,
                            void* win_row, void* win_src, void* row_win, size_t* widest, void* stream,
                            double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0;
  shred::EncodeDevice::BatchOpts o;
  if (window_args(enc, ids, n, row_off, rows, bos, eos, max_len, stride, pad_side, win_row, &o)) return -1;
  return enc->dev->window((const int32_t*)ids, n, (const int64_t*)row_off, rows, o, stride, width, pad_id, pad_side,
                          (int32_t*)out, cap, (int32_t*)lengths, (uint8_t*)mask, (int32_t*)win_row, (int64_t*)win_src,
                          (int64_t*)row_win, widest, stream, kernel_ms);
}

int64_t shred_window_rows(ShredEncoder* enc, const int32_t* ids, size_t n, const int64_t* row_off, size_t rows,
                          const int32_t* bos, const int32_t* eos, size_t max_len, size_t stride, size_t width,
                          int32_t pad_id, int pad_side, int32_t* out, size_t cap, int32_t* lengths, uint8_t* mask,
                          int32_t* win_row, int64_t* win_src, int64_t* row_win, size_t* widest) {
  shred::EncodeDevice::BatchOpts o;
  if (window_args(enc, ids, n, row_off, rows, bos, eos, max_len, stride, pad_side, win_row, &o)) return -1;
  // the length pass of host rows: max_len bounds every window, so only row_off can be wrong
  uint64_t total = 0, first = 0;
  if (const int r = batch_host_lengths(n, row_off, rows, o, &total, &first)) return r;
  const uint64_t add = (bos ? 1 : 0) + (eos ? 1 : 0), C = max_len - add, step = C - stride;
  const uint64_t R = row_off ? rows : 1;
  uint64_t Wn = 0;
  for (size_t r = 0; r < R; ++r)
    Wn += shred::window_count(row_off ? (uint64_t)(row_off[r + 1] - row_off[r]) : (uint64_t)n, C, step);
  if (Wn > (uint64_t)INT64_MAX || (width && Wn > (uint64_t)INT64_MAX / width)) return -1;
  if (widest) *widest = (size_t)first;
  if (!out || width < first || cap < Wn * width) return (int64_t)Wn;
  const int r = enc->dev->window_host(ids, n, row_off, rows, o, stride, width, pad_id, pad_side, out, lengths, mask,
                                      win_row, win_src, row_win);
  return r < 0 ? r : (int64_t)Wn;
}

namespace {
// What the two pair calls refuse before any work (0 or -1), and their options.
int pair_args(const ShredEncoder* enc, const void* ids_a, size_t n_a, const void* row_a, const void* ids_b, size_t n_b,
              const void* row_b, size_t rows, const int32_t* bos, const int32_t* mid, size_t mid_n, const int32_t* eos,
              size_t max_len, int trunc_side, int strategy, size_t max_a, size_t stride, int pad_side,
              const void* win_row, shred::EncodeDevice::PairOpts* o) {
  if (!enc || (n_a && !ids_a) || (n_b && !ids_b) || !row_a || !row_b || trunc_side < 0 || trunc_side > 1 ||
      pad_side < 0 || pad_side > 1 || mid_n > 2 || (mid_n && !mid) || strategy < 0 || strategy > 3)
    return -1;
  const size_t add = (bos ? 1 : 0) + mid_n + (eos ? 1 : 0);
  if (max_len && max_len < add) return -1;
  if (strategy != 3 && (stride || max_a)) return -1;
  if (strategy == 3) {
    if (!max_len || max_len > (size_t)INT32_MAX) return -1;
    const size_t B = max_len - add;
    if (max_a && (B < max_a || B - max_a <= stride)) return -1;
  }
  if (win_row && rows > (size_t)INT32_MAX) return -1;
  *o = shred::EncodeDevice::PairOpts{bos != nullptr, eos != nullptr, bos ? *bos : 0, eos ? *eos : 0,
                                     {mid_n > 0 ? mid[0] : 0, mid_n > 1 ? mid[1] : 0}, (uint32_t)mid_n,
                                     (uint64_t)max_len, trunc_side, strategy, (uint64_t)max_a, (uint64_t)stride};
  return 0;
}

// The length pass of host examples: 0 with Wn and the longest emitted row, -6 for a bad row_a or
// row_b, -7 for an example that cannot fit, -1 for an e past int32.
int pair_host_lengths(const shred::Pairs& pr, size_t rows, uint64_t* Wn, uint64_t* widest) {
  *Wn = *widest = 0;
  if (!offsets_ok(pr.ra, rows, pr.na) || !offsets_ok(pr.rb, rows, pr.nb)) return -6;
  bool too_long = false;
  for (size_t r = 0; r < rows; ++r) {
    uint64_t ka, kb;
    if (!pr.first((uint64_t)(pr.ra[r + 1] - pr.ra[r]), (uint64_t)(pr.rb[r + 1] - pr.rb[r]), &ka, &kb)) return -7;
    too_long |= pr.too_long(ka, kb);
    *widest = std::max(*widest, pr.add() + ka + kb);
    *Wn += pr.count(r);
  }
  return too_long ? -1 : 0;
}
}  // namespace

int64_t shred_pair_device(ShredEncoder* enc, const void* ids_a, size_t n_a, const void* row_a, const void* ids_b,
                          size_t n_b, const void* row_b, size_t rows, const int32_t* bos, const int32_t* mid,
                          size_t mid_n, const int32_t* eos, size_t max_len, int trunc_side, int strategy, size_t max_a,
                          size_t stride, size_t width, int32_t pad_id, int pad_side, void* out, size_t cap, void* types,
                          void* mask, void* lengths, void* win_row, void* seg_len, void* seg_src, void* row_win,
                          size_t* widest, void* stream, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0;
  shred::EncodeDevice::PairOpts o;
  if (pair_args(enc, ids_a, n_a, row_a, ids_b, n_b, row_b, rows, bos, mid, mid_n, eos, max_len, trunc_side, strategy,
                max_a, stride, pad_side, win_row, &o))
    return -1;
  return enc->dev->pair((const int32_t*)ids_a, n_a, (const int64_t*)row_a, (const int32_t*)ids_b, n_b,
                        (const int64_t*)row_b, rows, o, width, pad_id, pad_side, (int32_t*)out, cap, (uint8_t*)types,
                        (uint8_t*)mask, (int32_t*)lengths, (int32_t*)win_row, (int32_t*)seg_len, (int64_t*)seg_src,
                        (int64_t*)row_win, widest, stream, kernel_ms);
}

int64_t shred_pair_rows(ShredEncoder* enc, const int32_t* ids_a, size_t n_a, const int64_t* row_a, const int32_t* ids_b,
                        size_t n_b, const int64_t* row_b, size_t rows, const int32_t* bos, const int32_t* mid,
                        size_t mid_n, const int32_t* eos, size_t max_len, int trunc_side, int strategy, size_t max_a,
                        size_t stride, size_t width, int32_t pad_id, int pad_side, int32_t* out, size_t cap,
                        uint8_t* types, uint8_t* mask, int32_t* lengths, int32_t* win_row, int32_t* seg_len,
                        int64_t* seg_src, int64_t* row_win, size_t* widest) {
  shred::EncodeDevice::PairOpts o;
  if (pair_args(enc, ids_a, n_a, row_a, ids_b, n_b, row_b, rows, bos, mid, mid_n, eos, max_len, trunc_side, strategy,
                max_a, stride, pad_side, win_row, &o))
    return -1;
  if (!shred::batch_rows_fit(rows)) return -1;
  uint64_t Wn = 0, first = 0;
  if (const int r = pair_host_lengths(shred::pairs_of(o, row_a, n_a, row_b, n_b), rows, &Wn, &first)) return r;
  if (Wn > (uint64_t)INT64_MAX || (width && Wn > (uint64_t)INT64_MAX / width)) return -1;
  if (widest) *widest = (size_t)first;
  if (!out || width < first || cap < Wn * width) return (int64_t)Wn;
  const int r = enc->dev->pair_host(ids_a, n_a, row_a, ids_b, n_b, row_b, rows, o, width, pad_id, pad_side, out, types,
                                    mask, lengths, win_row, seg_len, seg_src, row_win);
  return r < 0 ? r : (int64_t)Wn;
}

namespace {
// T(q) of the masking section, or ~0 for a q outside [0, 1] (NaN included).
uint64_t mlm_threshold(double q) { return q >= 0 && q <= 1 ? (uint64_t)(q * 4294967296.0) : ~0ull; }

// What the two masking calls refuse before any work (0, -1 or -4), and their options.
int mlm_args(const ShredEncoder* enc, const void* ids, size_t n, const void* row_off, size_t rows,
             const ShredMlmOpts* o, const void* starts, const void* out, const void* labels,
             shred::EncodeDevice::MaskOpts* m) {
  if (!enc || !o || (n && (!ids || !out || !labels)) || (!row_off && rows)) return -1;
  if (n && (labels == ids || labels == out)) return -1;
  const uint64_t t_sel = mlm_threshold(o->p), t_mask = mlm_threshold(o->p_mask), t_rand = mlm_threshold(o->p_random);
  if (t_sel == ~0ull || t_mask == ~0ull || t_rand == ~0ull || t_mask + t_rand > (1ull << 32)) return -1;
  if (o->protect_n > SHRED_MLM_MAX_PROTECT || (o->protect_n && !o->protect)) return -1;
  if (o->p_random > 0 && (o->rand_vocab < 1 || o->rand_vocab > (int64_t)INT32_MAX)) return -1;
  if (o->whole_word && n && !starts) return -1;
  if (o->whole_word && !enc->spans_ok) return -4;
  const int32_t sp_lo = (int32_t)(256 + enc->first.size());
  *m = shred::EncodeDevice::MaskOpts{o->index_base, o->seed, t_sel, t_mask, t_mask + t_rand,
                                     o->p_random > 0 ? (uint64_t)o->rand_vocab : 0, o->mask_id, o->ignore_id,
                                     sp_lo, (int32_t)(sp_lo + enc->num_specials), o->protect_specials != 0,
                                     o->whole_word != 0, (uint32_t)o->protect_n, {}};
  for (size_t i = 0; i < o->protect_n; ++i) m->protect[i] = o->protect[i];
  return 0;
}
}  // namespace

int64_t shred_mlm_device(ShredEncoder* enc, const void* ids, size_t n, const void* row_off, size_t rows,
                         const ShredMlmOpts* opts, const void* starts, void* out, void* labels, void* stream,
                         double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0;
  shred::EncodeDevice::MaskOpts o;
  if (const int r = mlm_args(enc, ids, n, row_off, rows, opts, starts, out, labels, &o)) return r;
  return enc->dev->mask((const int32_t*)ids, n, (const int64_t*)row_off, rows, o, (const int64_t*)starts, enc->lens,
                        (int32_t*)out, (int32_t*)labels, stream, kernel_ms);
}

int64_t shred_mlm_rows(ShredEncoder* enc, const int32_t* ids, size_t n, const int64_t* row_off, size_t rows,
                       const ShredMlmOpts* opts, const int64_t* starts, int32_t* out, int32_t* labels) {
  shred::EncodeDevice::MaskOpts o;
  if (const int r = mlm_args(enc, ids, n, row_off, rows, opts, starts, out, labels, &o)) return r;
  if (!shred::batch_rows_fit(rows)) return -1;
  if (row_off && !offsets_ok(row_off, rows, n)) return -6;
  return enc->dev->mask_host(ids, n, row_off, rows, o, starts, enc->lens, out, labels);
}

namespace {
// What the two span-corruption calls refuse before any work (0 or -1), and their options.
int corrupt_args(const ShredEncoder* enc, const void* ids, size_t n, const void* row_off, size_t rows,
                 const ShredCorruptOpts* o, const void* in_ids, const void* in_row_off, const void* tgt_ids,
                 const void* tgt_row_off, shred::EncodeDevice::CorruptOpts* c) {
  if (!enc || !o || (n && !ids) || (!row_off && rows)) return -1;
  if (in_ids && tgt_ids && (!in_row_off || !tgt_row_off)) return -1;
  if (n && (in_ids == ids || tgt_ids == ids)) return -1;
  const uint64_t t_start = mlm_threshold(o->p_start);
  if (t_start == ~0ull) return -1;
  if (o->len_n < 1 || o->len_n > SHRED_CORRUPT_MAX_SPAN || !o->len_cum) return -1;
  for (size_t i = 1; i < o->len_n; ++i)
    if (o->len_cum[i - 1] > o->len_cum[i]) return -1;
  if (o->len_cum[o->len_n - 1] != (1ull << 32)) return -1;
  if (o->sentinel_n < 0) return -1;
  if (o->sentinel_n > 0) {
    const int64_t last = (int64_t)o->sentinel_first + (int64_t)(o->sentinel_n - 1) * (int64_t)o->sentinel_step;
    if (last < (int64_t)INT32_MIN || last > (int64_t)INT32_MAX) return -1;
  }
  if (o->protect_n > SHRED_MLM_MAX_PROTECT || (o->protect_n && !o->protect)) return -1;
  const int fin = o->final_sentinel != 0;
  const int32_t sp_lo = (int32_t)(256 + enc->first.size());
  *c = shred::EncodeDevice::CorruptOpts{};
  c->index_base = o->index_base, c->seed = o->seed, c->t_start = t_start, c->len_n = (uint32_t)o->len_n;
  for (size_t i = 0; i < o->len_n; ++i) c->len_cum[i] = o->len_cum[i];
  c->sent_first = o->sentinel_first, c->sent_step = o->sentinel_step;
  c->rmax = o->sentinel_n > fin ? (uint64_t)(o->sentinel_n - fin) : 0;
  c->closing = fin && o->sentinel_n > 0;
  c->sp_lo = sp_lo, c->sp_hi = (int32_t)(sp_lo + enc->num_specials);
  c->protect_specials = o->protect_specials != 0, c->protect_n = (uint32_t)o->protect_n;
  for (size_t i = 0; i < o->protect_n; ++i) c->protect[i] = o->protect[i];
  return 0;
}
}  // namespace

int64_t shred_corrupt_device(ShredEncoder* enc, const void* ids, size_t n, const void* row_off, size_t rows,
                             const ShredCorruptOpts* opts, void* in_ids, size_t in_cap, void* in_row_off, void* in_src,
                             void* tgt_ids, size_t tgt_cap, void* tgt_row_off, size_t* tgt_n, void* stream,
                             double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0;
  shred::EncodeDevice::CorruptOpts o;
  if (const int r = corrupt_args(enc, ids, n, row_off, rows, opts, in_ids, in_row_off, tgt_ids, tgt_row_off, &o)) return r;
  return enc->dev->corrupt((const int32_t*)ids, n, (const int64_t*)row_off, rows, o, (int32_t*)in_ids, in_cap,
                           (int64_t*)in_row_off, (int64_t*)in_src, (int32_t*)tgt_ids, tgt_cap, (int64_t*)tgt_row_off,
                           tgt_n, stream, kernel_ms);
}

int64_t shred_corrupt_rows(ShredEncoder* enc, const int32_t* ids, size_t n, const int64_t* row_off, size_t rows,
                           const ShredCorruptOpts* opts, int32_t* in_ids, size_t in_cap, int64_t* in_row_off,
                           int64_t* in_src, int32_t* tgt_ids, size_t tgt_cap, int64_t* tgt_row_off, size_t* tgt_n) {
  shred::EncodeDevice::CorruptOpts o;
  if (const int r = corrupt_args(enc, ids, n, row_off, rows, opts, in_ids, in_row_off, tgt_ids, tgt_row_off, &o)) return r;
  if (!shred::batch_rows_fit(rows)) return -1;
  if (row_off && !offsets_ok(row_off, rows, n)) return -6;
  return enc->dev->corrupt_host(ids, n, row_off, rows, o, in_ids, in_cap, in_row_off, in_src, tgt_ids, tgt_cap,
                                tgt_row_off, tgt_n);
}

namespace {
// The scalar options of the FIM calls: 0 or -1.
int fim_opts(const ShredFimOpts* o, shred::EncodeDevice::FimOpts* f) {
  if (!o) return -1;
  const uint64_t t_fim = mlm_threshold(o->fim_rate), t_spm = mlm_threshold(o->spm_rate);
  if (t_fim == ~0ull || t_spm == ~0ull || o->min_len < 0) return -1;
  *f = shred::EncodeDevice::FimOpts{o->row_base, o->seed, t_fim, t_spm, o->min_len, o->pre_id, o->suf_id, o->mid_id};
  return 0;
}

// What the two token-level FIM calls refuse before any work (0 or -1), and their options.
int fim_args(const ShredEncoder* enc, const void* ids, size_t n, const void* row_off, size_t rows,
             const ShredFimOpts* o, const void* out_ids, const void* out_row_off, shred::EncodeDevice::FimOpts* f) {
  if (!enc || (n && !ids) || (!row_off && rows)) return -1;
  if (out_ids && !out_row_off) return -1;
  if (n && out_ids == ids) return -1;
  return fim_opts(o, f);
}

// The -8 case on the host: every triple all -1, or 0 <= a <= b <= L and a mode of 0 or 1.
bool fim_cuts_ok(const int64_t* cuts, const int64_t* row_off, size_t R, size_t n) {
  for (size_t r = 0; r < R; ++r) {
    const int64_t a = cuts[3 * r], b = cuts[3 * r + 1], m = cuts[3 * r + 2];
    const int64_t L = row_off ? row_off[r + 1] - row_off[r] : (int64_t)n;
    if (a == -1 && b == -1 && m == -1) continue;
    if (a < 0 || a > b || b > L || (m != 0 && m != 1)) return false;
  }
  return true;
}
}  // namespace

int64_t shred_fim_device(ShredEncoder* enc, const void* ids, size_t n, const void* row_off, size_t rows,
                         const ShredFimOpts* opts, const void* cuts, void* out_ids, size_t out_cap, void* out_row_off,
                         void* out_src, void* out_seg, void* row_info, void* stream, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0;
  shred::EncodeDevice::FimOpts o;
  if (const int r = fim_args(enc, ids, n, row_off, rows, opts, out_ids, out_row_off, &o)) return r;
  return enc->dev->fim((const int32_t*)ids, n, (const int64_t*)row_off, rows, o, (const int64_t*)cuts,
                       (int32_t*)out_ids, out_cap, (int64_t*)out_row_off, (int64_t*)out_src, (uint8_t*)out_seg,
                       (int64_t*)row_info, stream, kernel_ms);
}

int64_t shred_fim_rows(ShredEncoder* enc, const int32_t* ids, size_t n, const int64_t* row_off, size_t rows,
                       const ShredFimOpts* opts, const int64_t* cuts, int32_t* out_ids, size_t out_cap,
                       int64_t* out_row_off, int64_t* out_src, uint8_t* out_seg, int64_t* row_info) {
  shred::EncodeDevice::FimOpts o;
  if (const int r = fim_args(enc, ids, n, row_off, rows, opts, out_ids, out_row_off, &o)) return r;
  if (!shred::batch_rows_fit(rows)) return -1;
  if (row_off && !offsets_ok(row_off, rows, n)) return -6;
  if (cuts && !fim_cuts_ok(cuts, row_off, row_off ? rows : 1, n)) return -8;
  return enc->dev->fim_host(ids, n, row_off, rows, o, cuts, out_ids, out_cap, out_row_off, out_src, out_seg, row_info);
}

int shred_fim_cuts_device(ShredEncoder* enc, const void* text, size_t n, const void* doc_off, size_t docs,
                          const ShredFimOpts* opts, void* piece_off, void* doc_mode, void* stream, double* kernel_ms) {
  if (kernel_ms) *kernel_ms = 0;
  shred::EncodeDevice::FimOpts o;
  if (!enc || (n && !text) || (!doc_off && docs) || !piece_off || !doc_mode || fim_opts(opts, &o)) return -1;
  return enc->dev->fim_cuts((const uint8_t*)text, n, (const int64_t*)doc_off, docs, o, (int64_t*)piece_off,
                            (int8_t*)doc_mode, stream, kernel_ms);
}

}  // extern "C"
