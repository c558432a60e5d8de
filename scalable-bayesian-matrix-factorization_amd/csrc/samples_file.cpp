// samples_file.cpp -- the sample store's two files: the sample file (sbmf_save_samples /
// sbmf_load_samples / sbmf_samples_file_info) and the samples' hyperparameters'
// companion file (sbmf_save_samples_hyper / sbmf_load_samples_hyper / sbmf_samples_hyper_file_info;
// INTEGRATION.md 3e).  The store itself is samples.cpp's.
#include <sys/stat.h>

#include "ctx.h"

namespace {

// ------------------------------------------------------------------ the two formats
// Little-endian throughout (the only byte order this library is built for).  A format is its
// header: the noun of its messages, magic and version, the check of its fields (a message of its
// own) and the file size the header implies.
struct FileHeader {  // 40 bytes
    char magic[8];
    uint32_t version, precision, I, J, K, count, bias, reserved;
    static constexpr const char* noun = "sample file";
    static constexpr char kMagic[8] = {'S', 'B', 'M', 'F', 'S', 'M', 'P', '\n'};
    static constexpr uint32_t kVersion = 1;
    void check(const char* fn, const char* path) const {
        if (precision > SBMF_F32 || bias > 1 || K == 0 || K > 256 || count > 65535)
            sbmf::fail(SBMF_E_IO, "%s: %s has a bad header (precision %u, bias %u, K %u, count %u)", fn, path, precision, bias, K,
                       count);
    }
    uint64_t sample_bytes() const {
        const uint64_t ts = precision == SBMF_F32 ? 4 : 8;
        return ((uint64_t)I + J) * K * ts + (bias ? (1 + (uint64_t)I + J) * 8 : 0);
    }
    uint64_t file_bytes() const { return sizeof(FileHeader) + (uint64_t)count * 4 + (uint64_t)count * sample_bytes(); }
};
static_assert(sizeof(FileHeader) == 40, "the sample file's header is 40 bytes");

struct HyperHeader {  // 24 bytes
    char magic[8];
    uint32_t version, K, count, reserved;
    static constexpr const char* noun = "sample hyperparameter file";
    static constexpr char kMagic[8] = {'S', 'B', 'M', 'F', 'S', 'H', 'P', '\n'};
    static constexpr uint32_t kVersion = 1;
    void check(const char* fn, const char* path) const {
        if (K == 0 || K > 256 || count > 65535 || reserved != 0)
            sbmf::fail(SBMF_E_IO, "%s: %s has a bad header (K %u, count %u, reserved %u)", fn, path, K, count, reserved);
    }
    uint64_t file_bytes() const { return sizeof(HyperHeader) + (uint64_t)count * 4 + (uint64_t)count * (4 * (uint64_t)K + 1) * 8; }
};
static_assert(sizeof(HyperHeader) == 24, "the companion file's header is 24 bytes");

struct File {
    FILE* f = nullptr;
    ~File() {
        if (f) std::fclose(f);
    }
};

// opens `path`, reads and validates the header against the file's size; the stream is left
// behind the header
template <typename Header>
void open_file(const char* fn, const char* path, File& file, Header& h) {
    file.f = std::fopen(path, "rb");
    struct stat sb;
    if (!file.f || fstat(fileno(file.f), &sb) != 0) sbmf::fail(SBMF_E_IO, "%s: cannot open %s", fn, path);
    const uint64_t size = (uint64_t)sb.st_size;
    if (size < sizeof(Header) || std::fread(&h, sizeof(Header), 1, file.f) != 1)
        sbmf::fail(SBMF_E_IO, "%s: %s is truncated in its header: %llu bytes, a %s's header has %zu", fn, path,
                   (unsigned long long)size, Header::noun, sizeof(Header));
    if (std::memcmp(h.magic, Header::kMagic, sizeof Header::kMagic) != 0)
        sbmf::fail(SBMF_E_IO, "%s: %s is not a %s (bad magic)", fn, path, Header::noun);
    if (h.version != Header::kVersion)
        sbmf::fail(SBMF_E_IO, "%s: %s has the unknown format version %u; this build reads version %u", fn, path, h.version,
                   Header::kVersion);
    h.check(fn, path);
    const uint64_t want = h.file_bytes();
    if (size < want)
        sbmf::fail(SBMF_E_IO, "%s: %s is truncated in its body: %llu bytes, its header implies %llu", fn, path,
                   (unsigned long long)size, (unsigned long long)want);
    if (size > want)
        sbmf::fail(SBMF_E_IO, "%s: %s has %llu trailing bytes: %llu bytes, its header implies %llu", fn, path,
                   (unsigned long long)(size - want), (unsigned long long)size, (unsigned long long)want);
}

// one stored sample's tables and biases, without padding, as the store holds them
template <typename T>
void download_slot(sbmf_ctx* c, uint32_t p, std::vector<T>& U, std::vector<T>& V, std::vector<double>& bu,
                   std::vector<double>& bv) {
    const SampleStore& ss = c->samples;
    const size_t I = c->I, J = c->J, K = c->K, Kp = c->Kp;
    std::vector<T> h((I > J ? I : J) * Kp);
    auto table = [&](const sbmf::DBuf& d, size_t R, std::vector<T>& out) {
        HIPCHK(hipMemcpy(h.data(), d.as<T>() + (size_t)p * R * Kp, R * Kp * sizeof(T), hipMemcpyDeviceToHost));
        out.resize(R * K);
        for (size_t r = 0; r < R; ++r) std::copy(h.begin() + r * Kp, h.begin() + r * Kp + K, out.begin() + r * K);
    };
    table(ss.d_U, I, U);
    table(ss.d_V, J, V);
    if (c->bias) {
        bu.resize(I);
        bv.resize(J);
        HIPCHK(hipMemcpy(bu.data(), ss.d_bu.as<double>() + (size_t)p * I, I * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(bv.data(), ss.d_bv.as<double>() + (size_t)p * J, J * sizeof(double), hipMemcpyDeviceToHost));
    }
}

template <typename T>
void save_T(sbmf_ctx* c, FILE* f, const char* path) {
    const SampleStore& ss = c->samples;
    std::vector<T> U, V;
    std::vector<double> bu, bv;
    for (uint32_t s = 0; s < ss.count; ++s) {
        const uint32_t p = ss.slot(s);
        download_slot<T>(c, p, U, V, bu, bv);
        bool ok = std::fwrite(U.data(), sizeof(T), U.size(), f) == U.size() &&
                  std::fwrite(V.data(), sizeof(T), V.size(), f) == V.size();
        if (ok && c->bias)
            ok = std::fwrite(&ss.b0[p], sizeof(double), 1, f) == 1 && std::fwrite(bu.data(), sizeof(double), bu.size(), f) == bu.size() &&
                 std::fwrite(bv.data(), sizeof(double), bv.size(), f) == bv.size();
        if (!ok) sbmf::fail(SBMF_E_IO, "sbmf_save_samples: writing %s failed", path);
    }
}

template <typename T>
void load_T(sbmf_ctx* c, FILE* f, const char* path, uint32_t count) {
    SampleStore& ss = c->samples;
    const size_t I = c->I, J = c->J, K = c->K, Kp = c->Kp;
    std::vector<T> packed((I > J ? I : J) * K), h((I > J ? I : J) * Kp, T(0));
    std::vector<double> b(I > J ? I : J);
    auto rd = [&](void* dst, size_t size, size_t cnt) {
        if (std::fread(dst, size, cnt, f) != cnt) sbmf::fail(SBMF_E_IO, "sbmf_load_samples: reading %s failed", path);
    };
    for (uint32_t s = 0; s < count; ++s) {
        auto table = [&](sbmf::DBuf& d, size_t R) {
            rd(packed.data(), sizeof(T), R * K);
            for (size_t r = 0; r < R; ++r) std::copy(packed.begin() + r * K, packed.begin() + (r + 1) * K, h.begin() + r * Kp);
            HIPCHK(hipMemcpy(d.as<T>() + (size_t)s * R * Kp, h.data(), R * Kp * sizeof(T), hipMemcpyHostToDevice));
        };
        table(ss.d_U, I);
        table(ss.d_V, J);
        if (c->bias) {
            rd(&ss.b0[s], sizeof(double), 1);
            rd(b.data(), sizeof(double), I);
            HIPCHK(hipMemcpy(ss.d_bu.as<double>() + (size_t)s * I, b.data(), I * sizeof(double), hipMemcpyHostToDevice));
            rd(b.data(), sizeof(double), J);
            HIPCHK(hipMemcpy(ss.d_bv.as<double>() + (size_t)s * J, b.data(), J * sizeof(double), hipMemcpyHostToDevice));
        }
    }
}

}  // namespace

extern "C" {

int sbmf_save_samples(sbmf_ctx* ctx, const char* path) {
    API_BEGIN
    if (!ctx || !path) sbmf::fail(SBMF_E_ARG, "null argument");
    samples_ready(ctx, "sbmf_save_samples");
    const SampleStore& ss = ctx->samples;
    FileHeader h{};
    std::memcpy(h.magic, FileHeader::kMagic, sizeof h.magic);
    h.version = FileHeader::kVersion;
    h.precision = (uint32_t)ctx->cfg.precision;
    h.I = ctx->I;
    h.J = ctx->J;
    h.K = ctx->K;
    h.count = ss.count;
    h.bias = ctx->bias ? 1u : 0u;
    File file;
    file.f = std::fopen(path, "wb");
    if (!file.f) sbmf::fail(SBMF_E_IO, "sbmf_save_samples: cannot open %s for writing", path);
    std::vector<uint32_t> sweeps(ss.count);
    for (uint32_t s = 0; s < ss.count; ++s) sweeps[s] = ss.sweep[ss.slot(s)];
    if (std::fwrite(&h, sizeof h, 1, file.f) != 1 || std::fwrite(sweeps.data(), 4, sweeps.size(), file.f) != sweeps.size())
        sbmf::fail(SBMF_E_IO, "sbmf_save_samples: writing %s failed", path);
    ctx->cfg.precision == SBMF_F32 ? save_T<float>(ctx, file.f, path) : save_T<double>(ctx, file.f, path);
    const int rc = std::fclose(file.f);
    file.f = nullptr;
    if (rc != 0) sbmf::fail(SBMF_E_IO, "sbmf_save_samples: writing %s failed", path);
    API_END(ctx)
}

int sbmf_load_samples(sbmf_ctx* ctx, const char* path) {
    API_BEGIN
    const char* fn = "sbmf_load_samples";
    if (!ctx || !path) sbmf::fail(SBMF_E_ARG, "null argument");
    list_scope(ctx, "sample store", fn, false);
    File file;
    FileHeader h;
    open_file(fn, path, file, h);
    static const char* const prec[] = {"f64", "f32"};
    if (h.precision != (uint32_t)ctx->cfg.precision)
        sbmf::fail(SBMF_E_ARG, "%s: %s holds precision %s; this context computes in %s", fn, path, prec[h.precision],
                   prec[ctx->cfg.precision]);
    if (h.I != ctx->I) sbmf::fail(SBMF_E_ARG, "%s: %s holds num_users = %u; this context has %u", fn, path, h.I, ctx->I);
    if (h.J != ctx->J) sbmf::fail(SBMF_E_ARG, "%s: %s holds num_items = %u; this context has %u", fn, path, h.J, ctx->J);
    if (h.K != ctx->K) sbmf::fail(SBMF_E_ARG, "%s: %s holds num_factor K = %u; this context has K = %u", fn, path, h.K, ctx->K);
    if (h.bias != (ctx->bias ? 1u : 0u))
        sbmf::fail(SBMF_E_ARG, "%s: %s holds bias = %u (%s biases); this context's quirk set is %s", fn, path, h.bias,
                   h.bias ? "with" : "without", ctx->bias ? "biased (bias = 1)" : "unbiased (bias = 0)");
    if (h.count == 0) sbmf::fail(SBMF_E_ARG, "%s: %s holds no sample", fn, path);
    list_sync(ctx);
    SampleStore& ss = ctx->samples;
    if (ss.cap < h.count) {
        const uint32_t every = ss.every;
        ss.drop();
        try {
            ss.alloc(ctx, h.count, every);
        } catch (const sbmf::Error& e) {
            ss.drop();
            if (e.code == SBMF_E_NOMEM)
                sbmf::fail(SBMF_E_NOMEM, "%s: %u samples of %zu bytes need %zu bytes of device memory: %s", fn, h.count,
                           slot_bytes(ctx), (size_t)h.count * slot_bytes(ctx), e.msg.c_str());
            throw;
        }
    }
    ss.head = ss.count = ss.seen = 0;
    ss.has_hyper = false;  // the file holds none (sbmf_load_samples_hyper)
    std::vector<uint32_t> sweeps(h.count);
    if (std::fread(sweeps.data(), 4, h.count, file.f) != h.count) sbmf::fail(SBMF_E_IO, "%s: reading %s failed", fn, path);
    std::copy(sweeps.begin(), sweeps.end(), ss.sweep.begin());
    ctx->cfg.precision == SBMF_F32 ? load_T<float>(ctx, file.f, path, h.count) : load_T<double>(ctx, file.f, path, h.count);
    ss.count = h.count;
    API_END(ctx)
}

int sbmf_samples_file_info(const char* path, uint32_t* version, uint32_t* precision, uint32_t* num_users,
                           uint32_t* num_items, uint32_t* num_factor, uint32_t* count, uint32_t* bias, uint64_t* bytes) {
    sbmf_ctx* ctx = nullptr;
    API_BEGIN
    if (!path) sbmf::fail(SBMF_E_ARG, "null path");
    File file;
    FileHeader h;
    open_file("sbmf_samples_file_info", path, file, h);
    if (version) *version = h.version;
    if (precision) *precision = h.precision;
    if (num_users) *num_users = h.I;
    if (num_items) *num_items = h.J;
    if (num_factor) *num_factor = h.K;
    if (count) *count = h.count;
    if (bias) *bias = h.bias;
    if (bytes) *bytes = h.file_bytes();
    API_END(ctx)
}

// --- the samples' hyperparameters' file ----------------------------------------------------------
int sbmf_save_samples_hyper(sbmf_ctx* ctx, const char* path) {
    API_BEGIN
    const char* fn = "sbmf_save_samples_hyper";
    if (!ctx || !path) sbmf::fail(SBMF_E_ARG, "null argument");
    samples_ready(ctx, fn);
    const SampleStore& ss = ctx->samples;
    if (!ss.has_hyper) sbmf::fail(SBMF_E_STATE, "%s: the stored samples have no hyperparameters to save", fn);
    HyperHeader h{};
    std::memcpy(h.magic, HyperHeader::kMagic, sizeof h.magic);
    h.version = HyperHeader::kVersion;
    h.K = ctx->K;
    h.count = ss.count;
    File file;
    file.f = std::fopen(path, "wb");
    if (!file.f) sbmf::fail(SBMF_E_IO, "%s: cannot open %s for writing", fn, path);
    const size_t per = 4 * (size_t)ctx->K + 1;
    std::vector<uint32_t> sweeps(ss.count);
    std::vector<double> body(ss.count * per);
    for (uint32_t s = 0; s < ss.count; ++s) {
        const uint32_t p = ss.slot(s);
        sweeps[s] = ss.sweep[p];
        std::copy(ss.hyper.begin() + p * per, ss.hyper.begin() + (p + 1) * per, body.begin() + s * per);
    }
    bool ok = std::fwrite(&h, sizeof h, 1, file.f) == 1 && std::fwrite(sweeps.data(), 4, sweeps.size(), file.f) == sweeps.size() &&
              std::fwrite(body.data(), 8, body.size(), file.f) == body.size();
    const int rc = std::fclose(file.f);
    file.f = nullptr;
    if (!ok || rc != 0) sbmf::fail(SBMF_E_IO, "%s: writing %s failed", fn, path);
    API_END(ctx)
}

int sbmf_load_samples_hyper(sbmf_ctx* ctx, const char* path) {
    API_BEGIN
    const char* fn = "sbmf_load_samples_hyper";
    if (!ctx || !path) sbmf::fail(SBMF_E_ARG, "null argument");
    list_scope(ctx, "sample store", fn, false);
    File file;
    HyperHeader h;
    open_file(fn, path, file, h);
    samples_ready(ctx, fn);
    SampleStore& ss = ctx->samples;
    if (h.K != ctx->K) sbmf::fail(SBMF_E_ARG, "%s: %s holds num_factor K = %u; this context has K = %u", fn, path, h.K, ctx->K);
    if (h.count != ss.count) sbmf::fail(SBMF_E_ARG, "%s: %s holds count = %u samples; the store holds %u", fn, path, h.count, ss.count);
    const size_t per = 4 * (size_t)ctx->K + 1;
    std::vector<uint32_t> sweeps(h.count);
    std::vector<double> body(h.count * per);
    if (std::fread(sweeps.data(), 4, sweeps.size(), file.f) != sweeps.size() ||
        std::fread(body.data(), 8, body.size(), file.f) != body.size())
        sbmf::fail(SBMF_E_IO, "%s: reading %s failed", fn, path);
    for (uint32_t s = 0; s < h.count; ++s)
        if (sweeps[s] != ss.sweep[ss.slot(s)])
            sbmf::fail(SBMF_E_ARG, "%s: %s holds sweep index %u for sample %u; the store's sample %u is sweep %u", fn, path,
                       sweeps[s], s, s, ss.sweep[ss.slot(s)]);
    for (uint32_t s = 0; s < h.count; ++s)
        std::copy(body.begin() + s * per, body.begin() + (s + 1) * per, ss.hyper.begin() + ss.slot(s) * per);
    ss.has_hyper = true;
    API_END(ctx)
}

int sbmf_samples_hyper_file_info(const char* path, uint32_t* version, uint32_t* num_factor, uint32_t* count, uint64_t* bytes) {
    sbmf_ctx* ctx = nullptr;
    API_BEGIN
    if (!path) sbmf::fail(SBMF_E_ARG, "null path");
    File file;
    HyperHeader h;
    open_file("sbmf_samples_hyper_file_info", path, file, h);
    if (version) *version = h.version;
    if (num_factor) *num_factor = h.K;
    if (count) *count = h.count;
    if (bytes) *bytes = h.file_bytes();
    API_END(ctx)
}

}  // extern "C"
