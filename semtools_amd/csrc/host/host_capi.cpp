// host_capi.cpp -- extern "C" surface of the host layer (include/semtools_host.h).
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <unistd.h>

#include "../../../include/semtools_host.h"
#include "../common.h"
#include "host.h"
#include "host_internal.h"
#include "json.h"
#include "fmt.h"

using namespace semtools;

// The host layer runs on a group (host.h).  Entry points that take an smt_ctx wrap it in a one-rank group, for which
// every sharded call is its single-GPU counterpart.
struct GroupRef {
    smt_group *g = nullptr;
    bool owned = false;   // a one-rank group made around the caller's context (the context itself stays the caller's)
    GroupRef() = default;
    GroupRef(const GroupRef &) = delete;
    GroupRef &operator=(const GroupRef &) = delete;
    ~GroupRef() { if (owned && g) smt_group_destroy(g); }
    void wrap(smt_ctx *ctx)
    {
        if (smt_group_from_ctx(ctx, &g) != SMT_OK) throw semtools::Error(smt_last_error());
        owned = true;
    }
    void use(smt_group *group) { g = group; owned = false; }
};

struct smt_host_model {
    GroupRef group;                          // (declared first: destroyed after the model that lives on it)
    std::unique_ptr<search::StaticModel> m;
};

struct smt_host_session {
    smt_host_model *model = nullptr;
    std::unique_ptr<search::Embeddings> emb;
    std::vector<search::Document> docs;
    bool ignore_case = false;
};

namespace {

int fail(const std::exception &e)
{
    smt::set_error("%s", e.what());
    return SMT_E_INVALID;
}

char *dup_text(const std::string &s)
{
    char *p = (char *)malloc(s.size() + 1);
    if (!p) return nullptr;
    memcpy(p, s.data(), s.size());
    p[s.size()] = 0;
    return p;
}

search::SearchConfig make_config(uint64_t n_lines, uint64_t top_k, double max_distance, int ignore_case)
{
    search::SearchConfig c;
    c.n_lines = (size_t)n_lines;
    c.top_k = (size_t)top_k;
    if (!std::isnan(max_distance)) c.max_distance = max_distance;
    c.ignore_case = ignore_case != 0;
    return c;
}

// ---- minimal safetensors reader: u64 header length, JSON header, raw little-endian data
// dtype (SMT_TABLE_*) / shape / byte offset of the `embeddings` tensor (no data read: the table goes to the device as stored,
// StaticModel streams or preads it)
int safetensors_embeddings_span(const std::string &path, uint64_t &V, uint64_t &byte_offset)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) throw Error("cannot open " + path);
    uint64_t hlen = 0;
    f.read(reinterpret_cast<char *>(&hlen), 8);
    if (!f || hlen > (1ull << 30)) throw Error("bad safetensors header in " + path);
    std::string hdr(hlen, '\0');
    f.read(&hdr[0], (std::streamsize)hlen);
    const json::Value h = json::parse(hdr);
    const json::Value *t = h.get("embeddings");
    if (!t) throw Error("tensor 'embeddings' not found in " + path);
    const auto &shape = t->get("shape")->arr;
    if (shape.size() != 2 || shape[1].as_u64() != SMT_DIM) throw Error("'embeddings' must be [V, 256]");
    V = shape[0].as_u64();
    byte_offset = 8 + hlen + t->get("data_offsets")->arr[0].as_u64();
    const std::string dtype = t->get("dtype")->s;
    if (dtype == "F32") return SMT_TABLE_F32;
    if (dtype == "F16") return SMT_TABLE_F16;
    if (dtype == "I8") return SMT_TABLE_I8;   // model2vec-rs converts each byte `as i8 as f32` (no scale): so does K1
    throw Error("unsupported embeddings dtype " + dtype + " (F32, F16, I8)");
}

// IEEE binary16 -> f32 by value
float half_to_float(uint16_t h)
{
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, ex = (h >> 10) & 0x1Fu, man = h & 0x3FFu;
    uint32_t bits;
    if (ex == 0x1F) bits = sign | 0x7F800000u | (man << 13);
    else if (ex != 0) bits = sign | ((ex + 112u) << 23) | (man << 13);
    else if (man == 0) bits = sign;
    else {   // subnormal half: a normal f32
        int e = -1;
        uint32_t m = man;
        do { ++e; m <<= 1; } while (!(m & 0x400u));
        bits = sign | ((uint32_t)(112 - e) << 23) | ((m & 0x3FFu) << 13);
    }
    float f;
    memcpy(&f, &bits, 4);
    return f;
}

// the optional tensors of a vocabulary-quantised model: `mapping` [n_tokens] (I32 / I64 -> u32, a negative entry is an error) and
// `weights` [n_tokens] (F64 / F32 / F16 -> f32 by value); a tensor that is absent leaves its vector empty
void safetensors_token_arrays(const std::string &path, std::vector<uint32_t> &mapping, std::vector<float> &weights)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) throw Error("cannot open " + path);
    uint64_t hlen = 0;
    f.read(reinterpret_cast<char *>(&hlen), 8);
    if (!f || hlen > (1ull << 30)) throw Error("bad safetensors header in " + path);
    std::string hdr(hlen, '\0');
    f.read(&hdr[0], (std::streamsize)hlen);
    const json::Value h = json::parse(hdr);
    auto raw = [&](const json::Value *t, const char *name, size_t elem, uint64_t &n) {
        const auto &shape = t->get("shape")->arr;
        if (shape.size() != 1 || shape[0].as_u64() == 0 || shape[0].as_u64() > (1ull << 32)) throw Error(std::string("'") + name + "' must be a non-empty vector");
        n = shape[0].as_u64();
        const uint64_t b = t->get("data_offsets")->arr[0].as_u64(), e = t->get("data_offsets")->arr[1].as_u64();
        if (e - b != n * elem) throw Error(std::string("'") + name + "': data size does not match its shape");
        std::vector<unsigned char> buf(n * elem);
        f.seekg((std::streamoff)(8 + hlen + b));
        f.read(reinterpret_cast<char *>(buf.data()), (std::streamsize)buf.size());
        if (!f) throw Error(path + " is truncated");
        return buf;
    };
    if (const json::Value *t = h.get("mapping")) {
        const std::string dtype = t->get("dtype")->s;
        if (dtype != "I32" && dtype != "I64") throw Error("unsupported mapping dtype " + dtype + " (I32, I64)");
        uint64_t n = 0;
        const auto buf = raw(t, "mapping", dtype == "I64" ? 8 : 4, n);
        mapping.resize(n);
        for (uint64_t i = 0; i < n; ++i) {
            int64_t v;
            if (dtype == "I64") memcpy(&v, &buf[i * 8], 8);
            else { int32_t x; memcpy(&x, &buf[i * 4], 4); v = x; }
            if (v < 0 || v > (int64_t)0xFFFFFFFFll) throw Error("token " + std::to_string(i) + ": mapping entry " + std::to_string(v) + " is not a table row");
            mapping[i] = (uint32_t)v;
        }
    }
    if (const json::Value *t = h.get("weights")) {
        const std::string dtype = t->get("dtype")->s;
        if (dtype != "F64" && dtype != "F32" && dtype != "F16") throw Error("unsupported weights dtype " + dtype + " (F64, F32, F16)");
        uint64_t n = 0;
        const auto buf = raw(t, "weights", dtype == "F64" ? 8 : dtype == "F32" ? 4 : 2, n);
        weights.resize(n);
        for (uint64_t i = 0; i < n; ++i) {
            if (dtype == "F64") { double v; memcpy(&v, &buf[i * 8], 8); weights[i] = (float)v; }
            else if (dtype == "F32") memcpy(&weights[i], &buf[i * 4], 4);
            else { uint16_t v; memcpy(&v, &buf[i * 2], 2); weights[i] = half_to_float(v); }
        }
    }
}

}  // namespace

extern "C" {

static int host_model_create(smt_ctx *ctx, smt_group *group, const float *table, uint64_t V, int normalize, int tok_kind,
                             const char *vocab_path, const char *unk_token, smt_tokenize_cb cb, void *user, uint32_t unk_id,
                             uint32_t median_len, smt_host_model **out)
{
    if ((!ctx && !group) || !table || !out) { smt::set_error("null argument"); return SMT_E_INVALID; }
    *out = nullptr;
    try {
        std::unique_ptr<Tokenizer> tok;
        if (tok_kind == SMT_TOK_HASH) tok = make_hash_tokenizer(V);
        else if (tok_kind == SMT_TOK_VOCAB) tok = make_vocab_tokenizer(vocab_path ? vocab_path : "", unk_token ? unk_token : "");
        else if (tok_kind == SMT_TOK_CALLBACK) {
            if (!cb) { smt::set_error("callback tokenizer without a callback"); return SMT_E_INVALID; }
            TokenizeFn fn = [cb, user](const std::string &text, std::vector<uint32_t> &ids) {
                uint64_t n = 0;
                ids.resize(std::max<size_t>(64, text.size() + 8));
                if (cb(user, text.data(), text.size(), ids.data(), ids.size(), &n) != 0) throw Error("tokenizer callback failed");
                if (n > ids.size()) {
                    ids.resize(n);
                    if (cb(user, text.data(), text.size(), ids.data(), ids.size(), &n) != 0) throw Error("tokenizer callback failed");
                }
                ids.resize(n);
            };
            tok = make_callback_tokenizer(std::move(fn), V, unk_id == UINT32_MAX ? std::nullopt : std::optional<uint32_t>(unk_id),
                                          median_len ? median_len : 5);
        } else { smt::set_error("unknown tokenizer kind %d", tok_kind); return SMT_E_INVALID; }
        std::unique_ptr<smt_host_model> h(new smt_host_model());
        if (group) h->group.use(group); else h->group.wrap(ctx);
        h->m = std::make_unique<search::StaticModel>(h->group.g, std::move(tok), table, V, normalize != 0);
        *out = h.release();
        return SMT_OK;
    } catch (const std::exception &e) { return fail(e); }
}

int smt_host_model_create(smt_ctx *ctx, const float *table, uint64_t V, int normalize, int tok_kind, const char *vocab_path,
                          const char *unk_token, smt_tokenize_cb cb, void *user, uint32_t unk_id, uint32_t median_len,
                          smt_host_model **out)
{
    return host_model_create(ctx, nullptr, table, V, normalize, tok_kind, vocab_path, unk_token, cb, user, unk_id, median_len, out);
}

int smt_host_model_create_group(smt_group *group, const float *table, uint64_t V, int normalize, int tok_kind, const char *vocab_path,
                                const char *unk_token, smt_tokenize_cb cb, void *user, uint32_t unk_id, uint32_t median_len,
                                smt_host_model **out)
{
    return host_model_create(nullptr, group, table, V, normalize, tok_kind, vocab_path, unk_token, cb, user, unk_id, median_len, out);
}

// "0,1,2" = those GPUs (RCCL between them); "all" = every visible GPU; "<d>:<n>" = n logical shards on GPU d (a test rig
// with one GPU: device copies stand in for RCCL); "<d>" = GPU d alone.
int smt_host_group_from_spec(const char *spec, smt_group **out)
{
    if (!spec || !out) { smt::set_error("null argument"); return SMT_E_INVALID; }
    *out = nullptr;
    const std::string s(spec);
    if (s == "all") {
        const int n = smt_device_count();
        if (n <= 0) { if (n == 0) smt::set_error("no HIP device visible: libsemtools_hip has no CPU fallback"); return SMT_E_HIP; }
        if (n == 1) return smt_group_create_logical(0, 1, out);
        std::vector<int> devs;
        for (int i = 0; i < n; ++i) devs.push_back(i);
        return smt_group_create(devs.data(), n, out);
    }
    const size_t colon = s.find(':');
    char *end = nullptr;
    if (colon != std::string::npos) {
        const long dev = strtol(s.c_str(), &end, 10);
        const long n = strtol(s.c_str() + colon + 1, nullptr, 10);
        if (end != s.c_str() + colon || dev < 0 || n < 1) { smt::set_error("device spec '%s': expected <device>:<shards>", spec); return SMT_E_INVALID; }
        return smt_group_create_logical((int)dev, (int)n, out);
    }
    std::vector<int> devs;
    for (const char *p = s.c_str(); *p;) {
        const long d = strtol(p, &end, 10);
        if (end == p || d < 0 || (*end && *end != ',')) { smt::set_error("device spec '%s': expected a comma-separated list of GPU ordinals", spec); return SMT_E_INVALID; }
        devs.push_back((int)d);
        p = *end ? end + 1 : end;
    }
    if (devs.empty()) { smt::set_error("device spec is empty"); return SMT_E_INVALID; }
    if (devs.size() == 1) return smt_group_create_logical(devs[0], 1, out);   // one GPU: no communicator needed
    return smt_group_create(devs.data(), (int)devs.size(), out);
}

char *smt_host_timing_json(void) { return dup_text(search::PhaseTimer::json()); }

struct smt_host_tokenizer {
    std::unique_ptr<Tokenizer> t;
};

int smt_host_tokenizer_load(const char *tokenizer_json_path, smt_host_tokenizer **out)
{
    if (!tokenizer_json_path || !out) { smt::set_error("null argument"); return SMT_E_INVALID; }
    *out = nullptr;
    try {
        auto *h = new smt_host_tokenizer();
        h->t = make_hf_tokenizer(tokenizer_json_path);
        *out = h;
        return SMT_OK;
    } catch (const std::exception &e) { return fail(e); }
}

void smt_host_tokenizer_free(smt_host_tokenizer *tok) { delete tok; }

int smt_host_tokenizer_encode(smt_host_tokenizer *tok, const char *text, uint32_t *ids, uint64_t cap, uint64_t *n_ids)
{
    if (!tok || !text || !n_ids || (cap && !ids)) { smt::set_error("null argument"); return SMT_E_INVALID; }
    try {
        std::vector<uint32_t> v;
        tok->t->encode(text, v);
        *n_ids = v.size();
        for (uint64_t i = 0; i < std::min<uint64_t>(cap, v.size()); ++i) ids[i] = v[i];
        return v.size() > cap ? SMT_E_TRUNCATED : SMT_OK;
    } catch (const std::exception &e) { return fail(e); }
}

int smt_host_tokenizer_info(smt_host_tokenizer *tok, uint64_t *vocab_size, int64_t *unk_id, uint64_t *median_token_bytes)
{
    if (!tok) { smt::set_error("null argument"); return SMT_E_INVALID; }
    if (vocab_size) *vocab_size = tok->t->vocab_size();
    if (unk_id) *unk_id = tok->t->unk_id() ? (int64_t)*tok->t->unk_id() : -1;
    if (median_token_bytes) *median_token_bytes = tok->t->median_token_length();
    return SMT_OK;
}

int smt_host_model_set_device_tokenizer(smt_host_model *model, int on)
{
    if (!model) { smt::set_error("null argument"); return SMT_E_INVALID; }
    model->m->set_device_tokenizer(on);   // 0 off, 1 the ASCII forms, 2 the UTF-8 form where the tokenizer has one
    return SMT_OK;
}

int smt_host_model_set_device_tokenizer_long(smt_host_model *model, int on)
{
    if (!model) { smt::set_error("null argument"); return SMT_E_INVALID; }
    model->m->set_device_tokenizer_long(on != 0);   // a Unigram route keeps pieces up to SMT_UG_MAX_LONG raw bytes on the device
    return SMT_OK;
}

int smt_host_debug_device_tokenized(smt_host_model *model, uint64_t *lines)
{
    if (!model || !lines) { smt::set_error("null argument"); return SMT_E_INVALID; }
    *lines = model->m->device_tokenized_lines();
    return SMT_OK;
}

int smt_host_model_set_device_lower(smt_host_model *model, int on)
{
    if (!model) { smt::set_error("null argument"); return SMT_E_INVALID; }
    model->m->set_device_lower(on != 0);   // the lines of an ignore_case call are lowered on the device while the route serves them
    return SMT_OK;
}

int smt_host_debug_device_lowered(smt_host_model *model, uint64_t *lines)
{
    if (!model || !lines) { smt::set_error("null argument"); return SMT_E_INVALID; }
    *lines = model->m->device_lowered_lines();
    return SMT_OK;
}

int smt_host_tokenizer_to_device(smt_host_tokenizer *tok, smt_ctx *ctx, smt_wordpiece **out)
{
    if (!tok || !out) { smt::set_error("null argument"); return SMT_E_INVALID; }
    *out = nullptr;
    try {
        WordpieceExport x;
        if (!tok->t->export_wordpiece(x)) {
            smt::set_error("this tokenizer has no device form (pure-ASCII lines of BertNormalizer -> BertPreTokenizer -> WordPiece only)");
            return SMT_E_UNSUPPORTED;
        }
        const smt_wordpiece_params p = x.params();
        return smt_wordpiece_create(ctx, &p, out);   // (no context: SMT_E_HIP on a machine without a device)
    } catch (const std::exception &e) { return fail(e); }
}

int smt_host_tokenizer_to_device_utf8(smt_host_tokenizer *tok, smt_ctx *ctx, smt_wordpiece **out)
{
    if (!tok || !out) { smt::set_error("null argument"); return SMT_E_INVALID; }
    *out = nullptr;
    try {
        WordpieceUtf8Export x;
        if (!tok->t->export_wordpiece_utf8(x)) {
            smt::set_error("this tokenizer has no UTF-8 device form (BertNormalizer -> BertPreTokenizer -> WordPiece with an unk token and "
                           "ASCII added tokens only)");
            return SMT_E_UNSUPPORTED;
        }
        const smt_wordpiece_params p = x.base.params();
        const smt_wordpiece_codepoints cp = x.codepoints();
        return smt_wordpiece_create_utf8(ctx, &p, &cp, out);   // (no context: SMT_E_HIP on a machine without a device)
    } catch (const std::exception &e) { return fail(e); }
}

int smt_host_tokenizer_to_device_unigram(smt_host_tokenizer *tok, smt_ctx *ctx, smt_unigram **out)
{
    if (!tok || !out) { smt::set_error("null argument"); return SMT_E_INVALID; }
    *out = nullptr;
    try {
        UnigramExport x;
        if (!tok->t->export_unigram(x)) {
            smt::set_error("this tokenizer has no Unigram device form (pure-ASCII lines of a per-byte normalizer -> Metaspace -> Unigram only)");
            return SMT_E_UNSUPPORTED;
        }
        const smt_unigram_params p = x.params();
        const int rc = smt_unigram_create(ctx, &p, out);   // (no context: SMT_E_HIP on a machine without a device)
        return rc == SMT_OK ? smt_unigram_set_space_rules(*out, (int)x.collapse_runs, (int)x.drop_trailing) : rc;
    } catch (const std::exception &e) { return fail(e); }
}

int smt_host_tokenizer_to_device_unigram_utf8(smt_host_tokenizer *tok, smt_ctx *ctx, smt_unigram **out)
{
    if (!tok || !out) { smt::set_error("null argument"); return SMT_E_INVALID; }
    *out = nullptr;
    try {
        UnigramUtf8Export x;
        if (!tok->t->export_unigram_utf8(x)) {
            smt::set_error("this tokenizer has no UTF-8 Unigram device form (a per-character normalizer -> Metaspace -> Unigram with ASCII "
                           "added tokens only)");
            return SMT_E_UNSUPPORTED;
        }
        const smt_unigram_params p = x.base.params();
        const smt_wordpiece_codepoints cp = x.codepoints();
        const int rc = smt_unigram_create_utf8(ctx, &p, &cp, out);   // (no context: SMT_E_HIP on a machine without a device)
        return rc == SMT_OK ? smt_unigram_set_space_rules(*out, (int)x.base.collapse_runs, (int)x.base.drop_trailing) : rc;
    } catch (const std::exception &e) { return fail(e); }
}

int smt_host_tokenizer_unigram_space_rules(smt_host_tokenizer *tok, int *collapse_runs, int *drop_trailing)
{
    if (!tok) { smt::set_error("null argument"); return SMT_E_INVALID; }
    try {
        UnigramExport x;
        if (!tok->t->export_unigram(x)) {
            smt::set_error("this tokenizer has no Unigram device form (pure-ASCII lines of a per-byte normalizer -> Metaspace -> Unigram only)");
            return SMT_E_UNSUPPORTED;
        }
        if (collapse_runs) *collapse_runs = (int)x.collapse_runs;
        if (drop_trailing) *drop_trailing = (int)x.drop_trailing;
        return SMT_OK;
    } catch (const std::exception &e) { return fail(e); }
}

static int host_model_from_dir(smt_ctx *ctx, smt_group *group, const char *dir, smt_host_model **out)
{
    if ((!ctx && !group) || !dir || !out) { smt::set_error("null argument"); return SMT_E_INVALID; }
    *out = nullptr;
    try {
        const std::string d(dir);
        search::PhaseTimer::mark("process_start_and_hip_context");   // (everything before the model directory is touched)
        uint64_t V = 0, table_offset = 0;
        // the table streams file -> pinned -> HBM (or is read row by row: StaticModel's lazy mode) in the dtype it is stored in
        const int table_dtype = safetensors_embeddings_span(d + "/model.safetensors", V, table_offset);
        bool normalize = true;
        std::string unk = "[UNK]";
        try {
            const json::Value cfg = json::parse(read_to_string(d + "/config.json"));
            if (auto *x = cfg.get("normalize")) normalize = x->b;
            if (auto *x = cfg.get("unk_token")) unk = x->s;
        } catch (const std::exception &) {}
        // a real model2vec directory carries tokenizer.json (read natively: hf_tokenizer.cpp); the synthetic test
        // models carry a plain vocab.txt
        std::unique_ptr<Tokenizer> tok;
        {
            std::ifstream tj(d + "/tokenizer.json");
            if (tj.good()) tok = make_hf_tokenizer(d + "/tokenizer.json");
            else tok = make_vocab_tokenizer(d + "/vocab.txt", unk);
        }
        // a vocabulary-quantised model: token id -> row and a scalar per token; the vocabulary is then checked against n_tokens
        std::vector<uint32_t> mapping;
        std::vector<float> weights;
        safetensors_token_arrays(d + "/model.safetensors", mapping, weights);
        const bool indexed = !mapping.empty() || !weights.empty();
        if (!mapping.empty() && !weights.empty() && mapping.size() != weights.size()) throw Error("'mapping' and 'weights' differ in length");
        const uint64_t n_tokens = !mapping.empty() ? mapping.size() : !weights.empty() ? weights.size() : V;
        if (mapping.empty() && n_tokens != V) throw Error("'weights' without 'mapping' must have one entry per embedding row");
        if (tok->vocab_size() > n_tokens)
            throw Error(indexed ? "the vocabulary has more tokens than 'mapping' / 'weights' have entries"
                                : "vocab.txt has more tokens than the embedding table has rows");
        search::PhaseTimer::mark("tokenizer_load");
        std::unique_ptr<smt_host_model> h(new smt_host_model());
        if (group) h->group.use(group); else h->group.wrap(ctx);
        if (indexed)
            h->m = std::make_unique<search::StaticModel>(h->group.g, std::move(tok), d + "/model.safetensors", table_offset, V, normalize, table_dtype,
                                                         std::move(mapping), std::move(weights));
        else
            h->m = std::make_unique<search::StaticModel>(h->group.g, std::move(tok), d + "/model.safetensors", table_offset, V, normalize, table_dtype);
        *out = h.release();
        return SMT_OK;
    } catch (const std::exception &e) { return fail(e); }
}

int smt_host_model_from_dir(smt_ctx *ctx, const char *dir, smt_host_model **out) { return host_model_from_dir(ctx, nullptr, dir, out); }
int smt_host_model_from_dir_group(smt_group *group, const char *dir, smt_host_model **out) { return host_model_from_dir(nullptr, group, dir, out); }

void smt_host_model_destroy(smt_host_model *model) { delete model; }

int smt_host_model_table_info(const smt_host_model *model, int *table_dtype, uint64_t *V, uint64_t *table_bytes, int *resident)
{
    if (!model || !model->m) { smt::set_error("null argument"); return SMT_E_INVALID; }
    try {
        bool res = false;
        model->m->table_info(table_dtype, V, table_bytes, &res);
        if (resident) *resident = res ? 1 : 0;
        return SMT_OK;
    } catch (const std::exception &e) { return fail(e); }
}

int smt_host_model_token_info(const smt_host_model *model, uint64_t *n_tokens, int *has_mapping, int *has_weights, uint64_t *token_bytes)
{
    if (!model || !model->m) { smt::set_error("null argument"); return SMT_E_INVALID; }
    try {
        bool hm = false, hw = false;
        model->m->token_info(n_tokens, &hm, &hw, token_bytes);
        if (has_mapping) *has_mapping = hm ? 1 : 0;
        if (has_weights) *has_weights = hw ? 1 : 0;
        return SMT_OK;
    } catch (const std::exception &e) { return fail(e); }
}

int smt_host_encode(smt_host_model *model, const char *const *texts, uint64_t n, uint32_t max_length, float *out)
{
    if (!model || (n && (!texts || !out))) { smt::set_error("null argument"); return SMT_E_INVALID; }
    try {
        std::vector<std::string> s(texts, texts + n);
        auto v = model->m->encode_with_args(s, max_length ? std::optional<size_t>(max_length) : std::nullopt, 16384);
        for (uint64_t i = 0; i < n; ++i) memcpy(out + i * SMT_DIM, v[i].data(), SMT_DIM * sizeof(float));
        return SMT_OK;
    } catch (const std::exception &e) { return fail(e); }
}

int smt_host_encode_lowered(smt_host_model *model, const char *const *texts, uint64_t n, uint32_t max_length, float *out)
{
    if (!model || (n && (!texts || !out))) { smt::set_error("null argument"); return SMT_E_INVALID; }
    try {
        std::vector<std::string> s(texts, texts + n);
        auto v = model->m->encode_with_args(s, max_length ? std::optional<size_t>(max_length) : std::nullopt, 16384, true);
        for (uint64_t i = 0; i < n; ++i) memcpy(out + i * SMT_DIM, v[i].data(), SMT_DIM * sizeof(float));
        return SMT_OK;
    } catch (const std::exception &e) { return fail(e); }
}

int smt_host_search_files(smt_host_model *model, const char *query, const char *const *files, uint64_t n_files, uint64_t n_lines,
                          uint64_t top_k, double max_distance, int ignore_case, int json, int is_tty, char **out_text)
{
    if (!model || !query || !out_text || (n_files && !files)) { smt::set_error("null argument"); return SMT_E_INVALID; }
    *out_text = nullptr;
    try {
        search::PhaseTimer::mark("between_calls");   // (a library caller's own time since the last phase is not split_lines)
        const auto cfg = make_config(n_lines, top_k, max_distance, ignore_case);
        const std::string q = ignore_case ? to_lowercase(query) : std::string(query);  // src/cmds/search.rs:130-134
        const auto res = search::search_files(std::vector<std::string>(files, files + n_files), q, *model->m, cfg);
        *out_text = dup_text(json ? cmds::search_results_json(res) : cmds::print_search_results(res, is_tty != 0));
        return SMT_OK;
    } catch (const std::exception &e) { return fail(e); }
}

int smt_host_search_content(smt_host_model *model, const char *query, const char *filename, const char *content, uint64_t n_lines,
                            uint64_t top_k, double max_distance, int ignore_case, int json, int is_tty, char **out_text)
{
    if (!model || !query || !content || !out_text) { smt::set_error("null argument"); return SMT_E_INVALID; }
    *out_text = nullptr;
    try {
        search::PhaseTimer::mark("between_calls");   // (a library caller's own time since the last phase is not split_lines)
        const auto cfg = make_config(n_lines, top_k, max_distance, ignore_case);
        const std::string q = ignore_case ? to_lowercase(query) : std::string(query);
        {
            search::Embeddings emb(model->m->group());
            std::vector<search::Document> docs;
            auto doc = search::create_document_from_content(filename ? filename : "<stdin>", std::string_view(content), *model->m, ignore_case != 0, emb);
            if (doc) docs.push_back(std::move(*doc));
            const auto res = search::search_documents(docs, emb, model->m->encode_single(q), cfg);
            *out_text = dup_text(json ? cmds::search_results_json(res) : cmds::print_search_results(res, is_tty != 0));
            search::PhaseTimer::mark("format_output");
        }
        search::PhaseTimer::mark("release_lines_and_rows");
        return SMT_OK;
    } catch (const std::exception &e) { return fail(e); }
}

int smt_host_search_workspace(smt_host_model *model, const char *query, const char *const *files, uint64_t n_files, uint64_t n_lines,
                              uint64_t top_k, double max_distance, int ignore_case, const char *workspace_name, int json, int is_tty,
                              char **out_text)
{
    if (!model || !query || !out_text || (n_files && !files)) { smt::set_error("null argument"); return SMT_E_INVALID; }
    *out_text = nullptr;
    try {
        search::PhaseTimer::mark("between_calls");   // (a library caller's own time since the last phase is not split_lines)
        const auto cfg = make_config(n_lines, top_k, max_distance, ignore_case);
        const std::string q = ignore_case ? to_lowercase(query) : std::string(query);
        std::optional<std::string> ws;
        if (workspace_name) ws = workspace_name;
        const auto ranked = search::search_with_workspace(std::vector<std::string>(files, files + n_files), q, *model->m, cfg, ws);
        *out_text = dup_text(json ? cmds::workspace_results_json(ranked, (size_t)n_lines)
                                  : cmds::print_workspace_search_results(ranked, (size_t)n_lines, is_tty != 0));
        return SMT_OK;
    } catch (const std::exception &e) { return fail(e); }
}

int smt_host_session_open(smt_host_model *model, const char *const *files, uint64_t n_files, int ignore_case, smt_host_session **out)
{
    if (!model || !out || (n_files && !files)) { smt::set_error("null argument"); return SMT_E_INVALID; }
    *out = nullptr;
    try {
        std::unique_ptr<smt_host_session> s(new smt_host_session());
        s->model = model;
        s->ignore_case = ignore_case != 0;
        s->emb = std::make_unique<search::Embeddings>(model->m->group());
        // (one embedding pipeline run over all files, like search_files: a repository is thousands of small files)
        s->docs = search::load_documents(std::vector<std::string>(files, files + n_files), *model->m, s->ignore_case, *s->emb);
        *out = s.release();
        return SMT_OK;
    } catch (const std::exception &e) { return fail(e); }
}

int smt_host_session_search(smt_host_session *s, const char *const *queries, uint64_t n_queries, uint64_t n_lines, uint64_t top_k,
                            double max_distance, int json, int is_tty, char **out_texts)
{
    if (!s || (n_queries && (!queries || !out_texts))) { smt::set_error("null argument"); return SMT_E_INVALID; }
    for (uint64_t i = 0; i < n_queries; ++i) out_texts[i] = nullptr;
    try {
        const auto cfg = make_config(n_lines, top_k, max_distance, s->ignore_case);
        std::vector<std::string> qs;
        for (uint64_t i = 0; i < n_queries; ++i) qs.push_back(s->ignore_case ? to_lowercase(queries[i]) : std::string(queries[i]));
        search::PhaseTimer::mark("between_session_calls");
        const auto qemb = s->model->m->encode_with_args(qs, 512, 1024);  // encode_single per query
        search::PhaseTimer::mark("session_encode_queries");
        const auto res = search::search_documents_batch(s->docs, *s->emb, qemb, cfg);
        search::PhaseTimer::mark("session_search_and_build_results");
        semtools::parallel_slices((size_t)n_queries, 128, [&](size_t b, size_t e) {
            for (size_t i = b; i < e; ++i)
                out_texts[i] = dup_text(json ? cmds::search_results_json(res[i]) : cmds::print_search_results(res[i], is_tty != 0));
        });
        search::PhaseTimer::mark("session_format");
        return SMT_OK;
    } catch (const std::exception &e) { return fail(e); }
}

uint64_t smt_host_session_lines(const smt_host_session *s) { return s ? s->emb->rows() : 0; }
void smt_host_session_close(smt_host_session *s) { delete s; }

static int host_workspace_use(smt_ctx *ctx, smt_group *group, const char *name, int json_out, char **out_text)
{
    if (!name || !out_text) { smt::set_error("null argument"); return SMT_E_INVALID; }
    *out_text = nullptr;
    try {
        GroupRef gr;
        if (group) gr.use(group); else if (ctx) gr.wrap(ctx);
        workspace::Workspace ws;
        ws.config.name = name;
        ws.config.root_dir = workspace::Workspace::root_path(name);
        ws.save();
        std::string out;
        if (json_out) {
            size_t total = 0;
            if (gr.g) { try { total = workspace::Store::open(ws.config.root_dir, gr.g)->get_stats().total_documents; } catch (const std::exception &) {} }
            json::Value o = json::Value::object();  // WorkspaceOutput (src/json_mode.rs:41-46)
            o.set("name", json::Value::str(ws.config.name));
            o.set("root_dir", json::Value::str(ws.config.root_dir));
            o.set("total_documents", json::Value::uint(total));
            out = json::to_string_pretty(o) + "\n";
        } else {
            const std::string n(name);  // src/cmds/workspace.rs:46-53
            out = "Workspace '" + n + "' configured.\nTo activate it, run:\n  export SEMTOOLS_WORKSPACE=" + n +
                  "\n\nOr add this to your shell profile (.bashrc, .zshrc, etc.)\n\nOr use the `--workspace` option on the commands that support it\n";
        }
        *out_text = dup_text(out);
        return SMT_OK;
    } catch (const std::exception &e) { return fail(e); }
}

int smt_host_workspace_use(smt_ctx *ctx, const char *name, int json_out, char **out_text) { return host_workspace_use(ctx, nullptr, name, json_out, out_text); }
int smt_host_workspace_use_group(smt_group *group, const char *name, int json_out, char **out_text) { return host_workspace_use(nullptr, group, name, json_out, out_text); }

static int host_workspace_status(smt_ctx *ctx, smt_group *group, const char *name_or_null, int json_out, char **out_text)
{
    if ((!ctx && !group) || !out_text) { smt::set_error("null argument"); return SMT_E_INVALID; }
    *out_text = nullptr;
    try {
        GroupRef gr;
        if (group) gr.use(group); else gr.wrap(ctx);
        std::optional<std::string> nm;
        if (name_or_null) nm = name_or_null;
        try { workspace::Workspace::active(nm); } catch (const Error &) { throw Error("No active workspace"); }
        const auto ws = workspace::Workspace::open(nm);
        const auto stats = workspace::Store::open(ws.config.root_dir, gr.g)->get_stats();
        std::string out;
        if (json_out) {
            json::Value o = json::Value::object();
            o.set("name", json::Value::str(ws.config.name));
            o.set("root_dir", json::Value::str(ws.config.root_dir));
            o.set("total_documents", json::Value::uint(stats.total_documents));
            out = json::to_string_pretty(o) + "\n";
        } else {  // src/cmds/workspace.rs:87-96
            out = "Active workspace: " + ws.config.name + "\nRoot: " + ws.config.root_dir + "\nDocuments: " +
                  std::to_string(stats.total_documents) + "\n";
            out += stats.has_index ? "Index: Yes (" + stats.index_type.value_or("Unknown") + ")\n" : "Index: No\n";
        }
        *out_text = dup_text(out);
        return SMT_OK;
    } catch (const std::exception &e) { return fail(e); }
}

int smt_host_workspace_status(smt_ctx *ctx, const char *name_or_null, int json_out, char **out_text) { return host_workspace_status(ctx, nullptr, name_or_null, json_out, out_text); }
int smt_host_workspace_status_group(smt_group *group, const char *name_or_null, int json_out, char **out_text) { return host_workspace_status(nullptr, group, name_or_null, json_out, out_text); }

int smt_host_workspace_reembed(smt_host_model *model, const char *name_or_null, int json_out, char **out_text)
{
    if (!model || !out_text) { smt::set_error("null argument"); return SMT_E_INVALID; }
    *out_text = nullptr;
    try {
        std::optional<std::string> nm;
        if (name_or_null) nm = name_or_null;
        try { workspace::Workspace::active(nm); } catch (const Error &) { throw Error("No active workspace"); }
        const auto ws = workspace::Workspace::open(nm);
        auto store = workspace::Store::open(ws.config.root_dir, model->m->group());
        const auto rep = store->reembed_from_token_cache(*model->m);
        std::string out;
        if (json_out) {
            json::Value o = json::Value::object();
            o.set("documents_reembedded", json::Value::uint(rep.documents));
            o.set("lines_reembedded", json::Value::uint(rep.lines));
            o.set("tokens_pooled", json::Value::uint(rep.tokens));
            json::Value miss = json::Value::array();
            for (auto &p : rep.missing) miss.arr.push_back(json::Value::str(p));
            o.set("documents_without_cached_tokens", std::move(miss));
            out = json::to_string_pretty(o) + "\n";
        } else if (!rep.missing.empty()) {
            out = "No cached tokens for " + std::to_string(rep.missing.size()) + " documents (nothing was changed):\n";
            for (auto &p : rep.missing) out += "  - " + p + "\n";
            out += "Search them once with this model to re-embed them from their files.\n";
        } else {
            out = "Re-embedded " + std::to_string(rep.lines) + " lines of " + std::to_string(rep.documents) +
                  " documents from cached tokens (" + std::to_string(rep.tokens) + " tokens).\n";
        }
        *out_text = dup_text(out);
        return SMT_OK;
    } catch (const std::exception &e) { return fail(e); }
}

static int host_workspace_prune(smt_ctx *ctx, smt_group *group, const char *name_or_null, int json_out, char **out_text)
{
    if ((!ctx && !group) || !out_text) { smt::set_error("null argument"); return SMT_E_INVALID; }
    *out_text = nullptr;
    try {
        GroupRef gr;
        if (group) gr.use(group); else gr.wrap(ctx);
        std::optional<std::string> nm;
        if (name_or_null) nm = name_or_null;
        try { workspace::Workspace::active(nm); } catch (const Error &) { throw Error("No active workspace"); }
        const auto ws = workspace::Workspace::open(nm);
        auto store = workspace::Store::open(ws.config.root_dir, gr.g);
        const auto all_paths = store->get_all_document_paths();
        std::vector<std::string> missing;
        for (auto &p : all_paths) if (access(p.c_str(), F_OK) != 0) missing.push_back(p);  // Path::exists()
        const size_t removed = missing.size(), remaining = all_paths.size() - removed;
        if (!missing.empty()) store->delete_documents(missing);
        std::string out;
        if (json_out) {
            json::Value o = json::Value::object();  // PruneOutput (src/json_mode.rs:48-52)
            o.set("files_removed", json::Value::uint(removed));
            o.set("files_remaining", json::Value::uint(remaining));
            out = json::to_string_pretty(o) + "\n";
        } else if (missing.empty()) {
            out = "No stale documents found. Workspace is clean.\n";
        } else {  // src/cmds/workspace.rs:148-157
            out = "Found " + std::to_string(removed) + " stale documents:\n";
            for (auto &p : missing) out += "  - " + p + "\n";
            out += "Removed " + std::to_string(removed) + " stale documents from workspace.\n";
        }
        *out_text = dup_text(out);
        return SMT_OK;
    } catch (const std::exception &e) { return fail(e); }
}

int smt_host_workspace_prune(smt_ctx *ctx, const char *name_or_null, int json_out, char **out_text) { return host_workspace_prune(ctx, nullptr, name_or_null, json_out, out_text); }
int smt_host_workspace_prune_group(smt_group *group, const char *name_or_null, int json_out, char **out_text) { return host_workspace_prune(nullptr, group, name_or_null, json_out, out_text); }

void smt_host_free(char *text) { free(text); }

char *smt_host_format_float(double value, int mode)
{
    if (mode == 0) return dup_text(fmt::rust_display(value));
    if (mode == 1) return dup_text(fmt::rust_display((float)value));
    return dup_text(fmt::json_f64(value));
}

char *smt_host_split_lines(const char *content)
{
    const auto lines = lines_of(content ? content : "");
    std::string out = std::to_string(lines.size());  // "<count>\x1f<line>\x1f<line>..."
    for (auto &l : lines) { out.push_back('\x1f'); out += l; }
    return dup_text(out);
}

char *smt_host_to_lowercase(const char *text) { return dup_text(to_lowercase(text ? text : "")); }

}  // extern "C"
