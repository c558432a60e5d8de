// loader.cpp -- every file the library reads and writes (host side of the boundary).
//
// Read:
// * SBPMF triples (sbmf_load_triples): a line is a rating iff sscanf(line, "%u%c%u%c%lf") >= 5
//   (gibbs_sbpmf_final.cpp:43,86,107,136,202); other lines are skipped.  The common "digits SEP
//   digits SEP number" shape is parsed directly and any other line goes through sscanf itself, so
//   acceptance is identical.
// * libFM text, "target id:value id:value ..." (Data.h:192-217): leading blanks skipped, empty and
//   '#' lines skipped, target read as DATA_FLOAT (float, fm_data.h:25), anything unparsable is an
//   error.  One tokenizer, two sinks: rating data (sbmf_load_libfm: exactly two features per line,
//   user id, then item id) and cases with any number of features (sbmf_load_libfm_cases).
// * libFM's binary sparse matrix with its target vector, row-major <stem>.x + <stem>.y
//   (sbmf_load_libfm_binary) or transposed <stem>.xt + <stem>.y (sbmf_load_libfm_binary_t), under
//   either of Data::load's two sets of names (sbmf_libfm_binary_kind, sbmf_load_libfm_data).
// * -meta's group file (sbmf_load_libfm_meta): one unsigned integer per attribute.
// * a block-structure relation (sbmf_load_libfm_relation): the block table <stem>.xt or <stem>.x,
//   the row maps <stem>.train / <stem>.test as text or as a binary DVector<uint>, and <stem>.groups.
// Written: triples (sbmf_save_triples), <stem>.x + .y (sbmf_save_libfm_binary), <stem>.xt + .y
// (sbmf_save_libfm_binary_t), a block table (sbmf_save_libfm_block) and a row map in either form
// (sbmf_save_libfm_row_map).
//
// The reference parses text in three serial passes (gibbs_sbpmf_final.cpp:26-215); here the file is
// read once and cut at line boundaries into one chunk per thread, each chunk parsed into its own
// arrays, and the chunks concatenated in file order -- the same ratings in the same order as a
// serial parse.  Numbers: "digits[.digits]" with a mantissa below 2^53 (2^24 for float) and at most
// 22 (10) fraction digits is m / 10^k, one correctly rounded division of two exactly representable
// values -- the value strtod (strtof) returns (Clinger's fast path); anything else goes through
// strtod / strtof itself.
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <thread>
#include <vector>

#include "../../include/sbmf.h"

namespace {

thread_local std::string g_lerr;

int fail(std::string msg, int code = SBMF_E_IO) {
    g_lerr = std::move(msg);
    return code;
}

// ---- memory, threads, whole files

// Large buffers on transparent huge pages where the kernel offers them (madvise
// mode): the first touch of a few hundred MB then takes hundreds of faults
// instead of ~10^5 (measured 1.05 -> see DESIGN §6 on a VM host).  free()able.
void* big_alloc(size_t bytes) {
    constexpr size_t HP = 2u << 20;
    if (bytes < HP) return std::malloc(bytes);
    void* p = std::aligned_alloc(HP, (bytes + HP - 1) / HP * HP);
    if (p) (void)madvise(p, (bytes + HP - 1) / HP * HP, MADV_HUGEPAGE);
    return p;
}

// user / item / rating for n ratings (one slot when n = 0); false with *out freed when one fails
bool alloc_ratings(sbmf_ratings* out, size_t n) {
    const size_t m = n ? n : 1;
    out->user = static_cast<uint32_t*>(big_alloc(m * sizeof(uint32_t)));
    out->item = static_cast<uint32_t*>(big_alloc(m * sizeof(uint32_t)));
    out->rating = static_cast<double*>(big_alloc(m * sizeof(double)));
    if (out->user && out->item && out->rating) return true;
    sbmf_free_ratings(out);
    return false;
}

int nthreads() {
    int th = (int)std::thread::hardware_concurrency();
    if (const char* e = std::getenv("SBMF_LOAD_THREADS")) th = std::atoi(e);
    else if (const char* o = std::getenv("OMP_NUM_THREADS")) th = std::min(th, std::atoi(o));
    return std::max(1, std::min(th, 64));
}

template <class F>
void parallel_for(size_t n, F&& f) {
    std::vector<std::thread> ths;
    for (size_t c = 1; c < n; ++c) ths.emplace_back(f, c);
    if (n) f(0);
    for (auto& t : ths) t.join();
}

// The whole file into an uninitialised buffer (+ a terminating 0), read by
// several threads (pread of disjoint ranges).
struct FreeDel {
    void operator()(char* p) const { std::free(p); }
};
using CBuf = std::unique_ptr<char, FreeDel>;
bool read_par(const char* path, CBuf& buf, size_t& n) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long sz = std::ftell(f);
    n = sz > 0 ? (size_t)sz : 0;
    buf.reset(static_cast<char*>(big_alloc(n + 1)));
    if (!buf) {
        std::fclose(f);
        return false;
    }
    const int fd = fileno(f);
    const size_t nt = std::max<size_t>(1, std::min<size_t>((size_t)nthreads(), n >> 24));
    std::vector<char> ok(nt, 1);
    parallel_for(nt, [&](size_t t) {
        size_t at = n * t / nt;
        const size_t e = n * (t + 1) / nt;
        while (at < e) {
            const ssize_t got = pread(fd, buf.get() + at, e - at, (off_t)at);
            if (got <= 0) {
                ok[t] = 0;
                return;
            }
            at += (size_t)got;
        }
    });
    std::fclose(f);
    buf.get()[n] = 0;
    return std::all_of(ok.begin(), ok.end(), [](char x) { return x != 0; });
}

// A whole input file, read-only: mapped (MAP_POPULATE: the page-cache pages are
// mapped in one pass, no copy) or, where mapping fails, read into a buffer.
struct InFile {
    const char* p = "";
    size_t n = 0;
    void* map = nullptr;
    CBuf buf;
    ~InFile() {
        if (map) munmap(map, n);
    }
};
bool open_in(const char* path, InFile& f) {
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return false;
    struct stat st;
    if (fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0) {
        void* m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE | MAP_POPULATE, fd, 0);
        if (m != MAP_FAILED) {
            close(fd);
            f.map = m;
            f.n = (size_t)st.st_size;
            f.p = static_cast<const char*>(m);
            return true;
        }
    }
    close(fd);
    if (!read_par(path, f.buf, f.n)) return false;
    f.p = f.buf.get();
    return true;
}

// ... or "unable to open <path>"
int open_or_fail(const std::string& path, InFile& f) {
    return open_in(path.c_str(), f) ? SBMF_OK : fail("unable to open " + path);
}

bool file_exists(const std::string& f) {
    FILE* h = std::fopen(f.c_str(), "rb");
    if (h) std::fclose(h);
    return h != nullptr;
}

// An output file: buffered writes that stop at the first failure, one verdict at close().
class OutFile {
    FILE* f = nullptr;
    bool good = false;

public:
    OutFile() = default;
    explicit OutFile(const std::string& path) { open(path); }
    OutFile(const OutFile&) = delete;
    ~OutFile() { close(); }
    bool open(const std::string& path) {
        f = std::fopen(path.c_str(), "wb");
        return good = f != nullptr;
    }
    void write(const void* p, size_t bytes) { good = good && (bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes); }
    bool ok() const { return good; }
    bool close() {
        if (f) good = (std::fclose(f) == 0) & good;
        f = nullptr;
        return good;
    }
};

// ---- numbers

inline bool parse_uint(const char*& p, unsigned& out) {
    if (*p < '0' || *p > '9') return false;
    unsigned long long v = 0;
    while (*p >= '0' && *p <= '9') {
        v = v * 10 + (unsigned)(*p - '0');
        if (v > 0xffffffffull) return false;
        ++p;
    }
    out = (unsigned)v;
    return true;
}

// "digits[.digits]" ending where strtod would stop (not at e/E/x/X/p/P/.):
// m / 10^k when exact operands make it strtod's correctly rounded result.
// Returns false (caller uses strtod / strtof) for every other form.
template <typename F>
inline bool parse_fast(const char* q, F& out, const char*& end) {
    constexpr unsigned long long MMAX = sizeof(F) == 8 ? (1ull << 53) : (1ull << 24);
    constexpr int KMAX = sizeof(F) == 8 ? 22 : 10;
    static const double p10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                   1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    const char* p = q;
    unsigned long long m = 0;
    int nd = 0, k = 0;
    while (*p >= '0' && *p <= '9') {
        m = m * 10 + (unsigned)(*p - '0');
        if (++nd > 18) return false;
        ++p;
    }
    if (nd == 0) return false;
    if (*p == '.') {
        ++p;
        while (*p >= '0' && *p <= '9') {
            m = m * 10 + (unsigned)(*p - '0');
            ++k;
            if (++nd > 18) return false;
            ++p;
        }
    }
    const char c = *p;
    if (c == 'e' || c == 'E' || c == 'x' || c == 'X' || c == 'p' || c == 'P' || c == '.') return false;
    if (m > MMAX || k > KMAX) return false;
    if (sizeof(F) == 8)
        out = (F)((double)m / p10[k]);
    else
        out = (F)((float)m / (float)p10[k]);
    end = p;
    return true;
}

inline bool is_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\f' || c == '\v'; }

// The next entry of a whitespace-separated list of unsigned integers below 2^32 - 1 (-meta's group
// ids, a text row map): 1 with the value, 0 at the end of the data, -1 where the entry is no such number.
int next_uint(const char*& q, const char* end, uint32_t& out) {
    while (q < end && is_space(*q)) ++q;
    if (q == end) return 0;
    uint64_t v = 0;
    const char* b = q;
    while (q < end && *q >= '0' && *q <= '9' && v <= 0xffffffffull) v = v * 10 + (uint64_t)(*q++ - '0');
    if (q == b || (q < end && !is_space(*q)) || v > 0xfffffffeull) return -1;
    out = (uint32_t)v;
    return 1;
}

// ---- text in line-aligned chunks

// What every chunk's parser keeps: the lines it saw and the first one it refused.
struct PartBase {
    size_t lines = 0;
    long err_line = -1;  // first bad line in the chunk (0-based within it)
    int err_code = SBMF_E_IO;
    std::string err;
};

// Line-aligned chunks of buf[0, n): one per thread, each at least SBMF_LOAD_CHUNK bytes
// (4 MiB unless set: smaller chunks are for tests).
std::vector<size_t> text_chunks(const char* buf, size_t n) {
    size_t min_bytes = 4u << 20;
    if (const char* e = std::getenv("SBMF_LOAD_CHUNK")) min_bytes = (size_t)std::max(1L, std::atol(e));
    const size_t want = std::max<size_t>(1, std::min<size_t>((size_t)nthreads(), n / min_bytes));
    std::vector<size_t> cut{0};
    for (size_t c = 1; c < want; ++c) {
        size_t at = std::max(cut.back(), n * c / want);
        const void* nl = at < n ? std::memchr(buf + at, '\n', n - at) : nullptr;
        at = nl ? (size_t)(static_cast<const char*>(nl) - buf) + 1 : n;
        if (at > cut.back() && at < n) cut.push_back(at);
    }
    cut.push_back(n);
    return cut;
}

// The first refused line over the parts in file order, as "<what> line N of <path>" with the file's
// line number; SBMF_OK when every part went through.
template <class Part>
int first_error(const std::vector<Part>& parts, const char* path) {
    size_t before = 0;
    for (const Part& p : parts) {
        if (p.err_line >= 0)
            return fail(p.err + " line " + std::to_string(before + (size_t)p.err_line + 1) + " of " + path, p.err_code);
        before += p.lines;
    }
    return SBMF_OK;
}

// The lines of a chunk over read-only bytes (a mapped file).  A line is [p, le) with le at its '\n'
// or at the end of the data; fast(p, le) reads at most up to that '\n' (a byte no number or id
// continues through), and the final line, which may have no '\n', is always parsed from a terminated
// copy.  Anything fast does not take goes to slow(copy), a terminated copy of the line parsed by the
// reference's own rule (sscanf / strtod / strtof / strtol), so acceptance and values are those of the
// serial parser.  The first line slow refuses ends the chunk.
template <class Fast, class Slow>
void walk_lines(PartBase& P, const char* p, const char* const end, Fast&& fast, Slow&& slow) {
    std::string tmp;
    while (p < end) {
        const char* nl = static_cast<const char*>(std::memchr(p, '\n', (size_t)(end - p)));
        const char* le = nl ? nl : end;
        const size_t lineno = P.lines++;
        if (!nl || !fast(p, le)) {
            tmp.assign(p, le);
            if (!slow(tmp.c_str())) {
                P.err_line = (long)lineno;
                return;
            }
        }
        p = le + 1;
    }
}

// A chunk's output for rating data: the ratings it parsed, written straight into the result
// arrays from slot `base` (its first line's index: a chunk never yields more
// ratings than lines), compacted afterwards.
struct Part : PartBase {
    uint32_t* u = nullptr;
    uint32_t* i = nullptr;
    double* r = nullptr;
    size_t n = 0;  // ratings parsed
    void push(uint32_t a, uint32_t b, double v) {
        u[n] = a;
        i[n] = b;
        r[n] = v;
        ++n;
    }
};

// Runs parse(part, begin, end) over the chunks on threads, each writing
// from its first line's slot, then closes the gaps in chunk order.
template <class F>
int run_chunks(const char* buf, size_t n, const char* path, F&& parse, sbmf_ratings* out) {
    const std::vector<size_t> cut = text_chunks(buf, n);
    const size_t nc = cut.size() - 1;
    // lines per chunk (a chunk ends after a newline, except possibly the last)
    std::vector<size_t> base(nc + 1, 0);
    parallel_for(nc, [&](size_t c) {
        size_t k = 0;
        const char* p = buf + cut[c];
        const char* const e = buf + cut[c + 1];
        while (p < e) {
            const void* nl = std::memchr(p, '\n', (size_t)(e - p));
            ++k;
            p = nl ? static_cast<const char*>(nl) + 1 : e;
        }
        base[c + 1] = k;
    });
    for (size_t c = 0; c < nc; ++c) base[c + 1] += base[c];
    if (!alloc_ratings(out, base[nc])) return SBMF_E_NOMEM;
    std::vector<Part> parts(nc);
    parallel_for(nc, [&](size_t c) {
        Part P;  // on the thread's own stack: its counters are written on every line
        P.u = out->user + base[c];
        P.i = out->item + base[c];
        P.r = out->rating + base[c];
        parse(P, buf + cut[c], buf + cut[c + 1]);
        parts[c] = std::move(P);
    });
    if (const int rc = first_error(parts, path)) {
        sbmf_free_ratings(out);
        return rc;
    }
    size_t total = 0;
    for (size_t c = 0; c < nc; ++c) {
        const Part& p = parts[c];
        if (total != base[c] && p.n) {  // close the gap left by skipped lines
            std::memmove(out->user + total, p.u, p.n * sizeof(uint32_t));
            std::memmove(out->item + total, p.i, p.n * sizeof(uint32_t));
            std::memmove(out->rating + total, p.r, p.n * sizeof(double));
        }
        total += p.n;
    }
    out->n = total;
    return SBMF_OK;
}

// ---- SBPMF triples: sscanf(line, "%u%c%u%c%lf") >= 5 (gibbs_sbpmf_final.cpp:43)

// fast path: digits SEP digits SEP <short decimal>
bool triple_fast(Part& P, const char* p, const char* le) {
    const char* q = p;
    unsigned a, b;
    double v;
    const char* e2;
    if (!parse_uint(q, a) || q >= le) return false;
    ++q;
    if (!parse_uint(q, b) || q >= le) return false;
    ++q;
    if (q >= le || *q == ' ' || *q == '\t' || !parse_fast(q, v, e2)) return false;
    P.push(a, b, v);
    return true;
}

bool triple_slow(Part& P, const char* t) {
    const char* q = t;
    unsigned a, b;
    if (parse_uint(q, a) && *q) {  // the direct form with strtod
        ++q;
        if (parse_uint(q, b) && *q) {
            ++q;
            if (*q && *q != ' ' && *q != '\t') {
                char* e2;
                errno = 0;
                const double v = std::strtod(q, &e2);
                if (e2 != q) {
                    P.push(a, b, v);
                    return true;
                }
            }
        }
    }
    unsigned uu, ii;
    char c1, c2;
    double v;
    if (std::sscanf(t, "%u%c%u%c%lf", &uu, &c1, &ii, &c2, &v) >= 5) P.push(uu, ii, v);  // the exact rule
    return true;  // any other line is skipped
}

// ---- libFM text (Data.h:192-217): one tokenizer over a sink that takes the line's features
//   Part& P                      the chunk's part (P.err names what a refused line lacks)
//   begin()                      a target was read, the features follow
//   feature(long id, float v)    false: the feature is refused, P.err set
//   end(float target, report)    the line is over: keeps the case; false: the case is refused, with
//                                P.err set when `report` (the slow path)
//   drop()                       forget the features since begin(): the fast path declines

// fast path over [p, le): short decimals and ids, blanks between, then the end of the line (or '#' /
// '\r'); false = take the slow path, which also reports whatever the sink refuses (nothing is kept)
template <class Sink>
inline bool libfm_fast(Sink& S, const char* p, const char* le) {
    const char* q = p;
    while (q < le && (*q == ' ' || *q == '\t')) ++q;
    if (q == le || *q == '#' || *q == '\r') return true;  // blank / comment line
    float target;
    const char* e;
    if (!parse_fast(q, target, e)) return false;
    q = e;
    S.begin();
    for (;;) {
        const char* b = q;
        while (q < le && (*q == ' ' || *q == '\t')) ++q;
        if (q >= le || *q == '#' || *q == '\r') break;
        unsigned id;
        float fv;
        if (q == b || !parse_uint(q, id) || id > 0x7fffffffu || q >= le || *q != ':' || !parse_fast(q + 1, fv, e) ||
            !S.feature((long)id, fv)) {
            S.drop();
            return false;
        }
        q = e;
    }
    if (S.end(target, false)) return true;
    S.drop();
    return false;
}

// the reference's rule on a terminated copy of the line (sscanf "%f", then "%d:%f" pairs).
// Returns false with P.err set on a bad line.
template <class Sink>
bool libfm_slow(Sink& S, const char* t) {
    const char* q = t;
    while (*q == ' ' || *q == '\t') ++q;
    if (*q == 0 || *q == '#' || *q == '\r') return true;
    char* e;
    const float target = std::strtof(q, &e);
    if (e == q) return S.P.err = "cannot parse libFM", false;
    q = e;
    S.begin();
    while (true) {
        while (*q == ' ' || *q == '\t') ++q;
        if (*q == 0 || *q == '#' || *q == '\r') break;
        char* e1;
        const long id = std::strtol(q, &e1, 10);
        if (e1 == q || *e1 != ':') return S.P.err = "cannot parse libFM", false;
        q = e1 + 1;
        char* e3;
        const float fv = std::strtof(q, &e3);
        if (e3 == q) return S.P.err = "cannot parse libFM", false;
        q = e3;
        if (!S.feature(id, fv)) return false;
    }
    return S.end(target, true);
}

template <class Sink>
void parse_libfm(Sink S, const char* p, const char* end) {
    walk_lines(S.P, p, end, [&S](const char* a, const char* le) { return libfm_fast(S, a, le); },
               [&S](const char* t) { return libfm_slow(S, t); });
}

// Rating data: the values are ignored, a line holds exactly the user's id, then the item's (the
// same id twice is two features), and the two ids stay in registers.
struct RatingSink {
    Part& P;
    const uint32_t item_offset;
    long id[2] = {0, 0};
    int nf = 0;
    void begin() { nf = 0; }
    bool feature(long a, float) {
        if (nf < 2) id[nf] = a;
        ++nf;
        return true;
    }
    bool end(float target, bool report) {
        if (nf != 2 || id[0] < 0 || id[1] < (long)item_offset || (item_offset > 0 && id[0] >= (long)item_offset)) {
            if (report)
                P.err = item_offset > 0 ? "the SBPMF sampler needs exactly one user and one item feature per line "
                                          "(user id < item_offset <= item id): libFM"
                                        : "the SBPMF sampler needs exactly one user and one item feature per line: libFM";
            return false;
        }
        P.push((uint32_t)id[0], (uint32_t)(id[1] - (long)item_offset), (double)target);
        return true;
    }
    void drop() {}
};

// Cases with any number of features per line (sbmf_cases): Data::load's text branch
// (Data.h:173-283).  Each chunk into vectors of its own, concatenated in file order.
struct CasePart : PartBase {
    std::vector<uint32_t> len, attr;  // features per case; the entries, case after case
    std::vector<float> x, y;
    uint32_t max_attr = 0;
    bool any = false;
};

// the entries pushed since `from`, sorted by id (stable); false on a repeated id
bool sort_case(CasePart& P, size_t from) {
    const size_t m = P.attr.size() - from;
    uint32_t* a = P.attr.data() + from;
    float* v = P.x.data() + from;
    bool sorted = true;
    for (size_t k = 1; k < m && sorted; ++k) sorted = a[k - 1] < a[k];
    if (sorted) return true;
    for (size_t k = 1; k < m; ++k) {  // insertion sort: stable, lines are short
        const uint32_t ka = a[k];
        const float kv = v[k];
        size_t j = k;
        for (; j > 0 && a[j - 1] > ka; --j) {
            a[j] = a[j - 1];
            v[j] = v[j - 1];
        }
        a[j] = ka;
        v[j] = kv;
    }
    for (size_t k = 1; k < m; ++k)
        if (a[k - 1] == a[k]) return false;
    return true;
}

struct CaseSink {
    CasePart& P;
    size_t from = 0;
    void begin() { from = P.attr.size(); }
    bool feature(long id, float v) {
        if (id < 0 || id > 0x7fffffffl) return P.err = "feature id out of range [0, 2^31) in libFM", false;
        P.attr.push_back((uint32_t)id);
        P.x.push_back(v);
        return true;
    }
    bool end(float target, bool) {
        if (!sort_case(P, from)) {
            P.err_code = SBMF_E_ARG;
            P.err = "an attribute id is repeated inside one case (the learner writes one record per case of a row):";
            return false;
        }
        for (size_t k = from; k < P.attr.size(); ++k) P.max_attr = std::max(P.max_attr, P.attr[k]);
        P.any = P.any || P.attr.size() > from;
        P.len.push_back((uint32_t)(P.attr.size() - from));
        P.y.push_back(target);
        return true;
    }
    void drop() {
        P.attr.resize(from);
        P.x.resize(from);
    }
};

// ---- libFM binary input: <stem>.x (or .data) + <stem>.y (or .target), the
// files tools/convert.cpp writes.  Layouts (fmatrix.h:36-52, matrix.h:280-328):
//   .x  file_header {u32 id = 2; u32 float_size = 4; u64 num_values; u32 num_rows;
//       u32 num_cols} (24 bytes, natural alignment), then per row u32 size and
//       size x sparse_entry {u32 id; f32 value}
//   .y  u32 version = 1; u32 float_size = 4; u32 num_rows; num_rows x f32
// Data::load (Data.h:113-160) prefers .data/.target over .x/.y and asserts
// target.dim == rows; the same order and checks apply here, as errors.
struct FmHeader {
    uint32_t id, float_size;
    uint64_t num_values;
    uint32_t num_rows, num_cols;
};
static_assert(sizeof(FmHeader) == 24, "fmatrix.h file_header layout");

// Data::load's file choice (Data.h:112-117), in its order of preference: the matrix, its transpose
// and the targets.  kind k of sbmf_libfm_binary_kind is NAMES[k - 1]; the writers write NAMES[1].
struct Names {
    const char *x, *xt, *y;
    const char* matrix(bool transposed) const { return transposed ? xt : x; }
};
const Names NAMES[2] = {{".data", ".datat", ".target"}, {".x", ".xt", ".y"}};
const Names& OWN = NAMES[1];

bool read_header(const std::string& path, const InFile& in, void* h, size_t bytes) {
    if (in.n < bytes) return fail(path + ": truncated header"), false;
    std::memcpy(h, in.p, bytes);
    return true;
}

// an opened sparse matrix file: its header, id 2 with 4-byte values
int matrix_header(const std::string& path, const InFile& in, FmHeader& h) {
    if (!read_header(path, in, &h, sizeof h)) return SBMF_E_IO;
    if (h.id != 2 || h.float_size != sizeof(float))
        return fail(path + ": not a libFM sparse matrix file (id 2, 4-byte values)");
    return SBMF_OK;
}

// an opened target file: version 1 with 4-byte values, all `n` of them present from byte 12
int target_header(const std::string& path, const InFile& in, uint32_t& n) {
    uint32_t h[3];
    if (!read_header(path, in, h, sizeof h)) return SBMF_E_IO;
    if (h[0] != 1 || h[1] != sizeof(float) || in.n < 12 + (size_t)h[2] * sizeof(float))
        return fail(path + ": not a libFM DVector<float> file (version 1, 4-byte values)");
    n = h[2];
    return SBMF_OK;
}

// The rows after a matrix's header: row(r, at, size) on each one that lies inside the file, `at` the
// offset of its size word, in file order; false from it ends the walk (the error is the caller's).
// A row cut short is reported as "truncated at <noun> r".  nv: the entries of the rows walked.
template <class F>
bool walk_rows(const std::string& path, const InFile& in, uint32_t num_rows, const char* noun, uint64_t& nv, F&& row) {
    size_t at = sizeof(FmHeader);
    nv = 0;
    for (uint32_t r = 0; r < num_rows; ++r) {
        uint32_t sz = 0;
        if (at + 4 > in.n || (std::memcpy(&sz, in.p + at, 4), at + 4 + (size_t)sz * 8 > in.n))
            return fail(path + ": truncated at " + noun + " " + std::to_string(r)), false;
        if (!row(r, at, sz)) return false;
        at += 4 + (size_t)sz * 8;
        nv += sz;
    }
    return true;
}

// A matrix with its targets, both opened (one message names the two), then the targets' header
// checked, then the matrix's.
struct Pair {
    InFile x, y;
    FmHeader h;
    uint32_t targets = 0;
    float target(size_t c) const {
        float t;
        std::memcpy(&t, y.p + 12 + c * 4, 4);
        return t;
    }
};
int open_pair(const std::string& xf, const std::string& yf, Pair& b) {
    if (!open_in(xf.c_str(), b.x) || !open_in(yf.c_str(), b.y)) return fail("unable to open " + xf + " / " + yf);
    const int rc = target_header(yf, b.y, b.targets);
    return rc != SBMF_OK ? rc : matrix_header(xf, b.x, b.h);
}

// rating data from the row-major file: every row {user, item}
int load_x(const std::string& xf, const std::string& yf, uint32_t item_offset, sbmf_ratings* out) {
    std::memset(out, 0, sizeof *out);
    Pair b;
    if (const int rc = open_pair(xf, yf, b)) return rc;
    const FmHeader& h = b.h;
    const char* const xb = b.x.p;
    if (h.num_rows != b.targets)
        return fail(xf + ": " + std::to_string(h.num_rows) + " rows but " + std::to_string(b.targets) + " targets");
    const size_t R = h.num_rows;
    if (!alloc_ratings(out, R)) return SBMF_E_NOMEM;
    auto bad_row = [&](uint64_t row) {
        sbmf_free_ratings(out);
        return fail(xf + " row " + std::to_string(row) +
                    ": the SBPMF sampler needs exactly one user and one item feature per row" +
                    (item_offset > 0 ? " (user id < item_offset <= item id)" : "") +
                    "; cases with any other number of features are read from libFM text only (sbmf_load_libfm_cases)");
    };
    auto take = [&](size_t row, const char* rec) -> bool {  // rec: {u32 size; 2 x {u32 id; f32 value}}
        uint32_t sz, f0, f1;
        std::memcpy(&sz, rec, 4);
        std::memcpy(&f0, rec + 4, 4);
        std::memcpy(&f1, rec + 12, 4);
        if (sz != 2 || f1 < item_offset || (item_offset > 0 && f0 >= item_offset)) return false;
        out->user[row] = f0;
        out->item[row] = f1 - item_offset;
        out->rating[row] = (double)b.target(row);
        return true;
    };
    // what the rating converter writes: every row {user, item}, 20 bytes, so row q
    // sits at 24 + 20 q -- rows taken in parallel; any other file is scanned row by row
    constexpr size_t REC = 4 + 2 * 8;
    if (b.x.n == sizeof h + R * REC && h.num_values == 2 * (uint64_t)R) {
        const size_t nt = std::max<size_t>(1, std::min<size_t>((size_t)nthreads(), R >> 18));
        std::vector<uint64_t> first_bad(nt, UINT64_MAX);
        parallel_for(nt, [&](size_t t) {
            for (size_t q = R * t / nt, e = R * (t + 1) / nt; q < e; ++q)
                if (!take(q, xb + sizeof h + q * REC)) {
                    first_bad[t] = q;
                    return;
                }
        });
        for (uint64_t q : first_bad)
            if (q != UINT64_MAX) return bad_row(q);
        out->n = R;
        return SBMF_OK;
    }
    uint64_t nv;
    const bool whole = walk_rows(xf, b.x, h.num_rows, "row", nv, [&](uint32_t row, size_t at, uint32_t sz) {
        return (sz == 2 && take(row, xb + at)) || (bad_row(row), false);
    });
    if (whole && nv != h.num_values)
        fail(xf + ": header says " + std::to_string(h.num_values) + " values, rows hold " + std::to_string(nv));
    if (!whole || nv != h.num_values) {
        sbmf_free_ratings(out);
        return SBMF_E_IO;
    }
    out->n = R;
    return SBMF_OK;
}

// libFM's transpose <stem>.xt + <stem>.y (or .datat + .target, preferred as
// Data::load does, Data.h:113-117,143-151): the file tools/transpose.cpp:54-172
// writes from a .x, with the .x header's roles swapped (num_rows = features,
// num_cols = cases) and one sparse row per feature {u32 size; size x {u32 case
// id; f32 value}}, case ids ascending.  This is the only file bin/libFM -method
// mcmc|als reads (has_x = false, libfm.cpp:140-149).  For rating data a
// feature's row is its user's or item's rating list, so the per-case pair is
// rebuilt: each case must hold exactly two features, the lower id is the user,
// the higher the item (users-first ids), and item_offset has the meaning of
// sbmf_load_libfm_binary.
int load_xt(const std::string& xf, const std::string& yf, uint32_t item_offset, sbmf_ratings* out) {
    std::memset(out, 0, sizeof *out);
    Pair b;
    if (const int rc = open_pair(xf, yf, b)) return rc;
    const FmHeader& h = b.h;
    const char* const xb = b.x.p;
    // the transpose's columns are the cases; Data::load takes num_cases from the
    // targets (Data.h:167), so the two must agree
    if (h.num_cols != b.targets)
        return fail(xf + ": " + std::to_string(h.num_cols) + " cases but " + std::to_string(b.targets) + " targets");
    const uint32_t F = h.num_rows;
    const size_t C = h.num_cols;
    // pass 1 (serial, one u32 per feature row): row offsets and the value count
    std::vector<size_t> off;
    off.reserve(std::min<size_t>(F, (b.x.n - sizeof h) / 4) + 1);  // a row takes 4 bytes or more
    uint64_t nv;
    if (!walk_rows(xf, b.x, F, "feature row", nv, [&](uint32_t, size_t at, uint32_t) { return off.push_back(at), true; }))
        return SBMF_E_IO;
    off.push_back(sizeof h + 4 * (size_t)F + 8 * (size_t)nv);
    if (nv != h.num_values)
        return fail(xf + ": header says " + std::to_string(h.num_values) + " values, rows hold " + std::to_string(nv));
    std::unique_ptr<std::atomic<uint32_t>[]> cnt(new (std::nothrow) std::atomic<uint32_t>[C ? C : 1]);
    if (!alloc_ratings(out, C) || !cnt) {
        sbmf_free_ratings(out);
        return SBMF_E_NOMEM;
    }
    const size_t nc = std::max<size_t>(1, std::min<size_t>((size_t)nthreads(), C >> 16));
    parallel_for(nc, [&](size_t t) {
        for (size_t c = C * t / nc, e = C * (t + 1) / nc; c < e; ++c) cnt[c].store(0, std::memory_order_relaxed);
    });
    // pass 2: feature rows cut into nt ranges of about equal value counts; a
    // case's first two features land in user[] / item[] in any order (sorted
    // below), a third one or a case id past the targets is an error
    const size_t nt = std::max<size_t>(1, std::min<size_t>((size_t)nthreads(), (size_t)(nv >> 17)));
    std::vector<uint32_t> fcut(nt + 1, F);
    fcut[0] = 0;
    for (size_t t = 1, f = 0; t < nt; ++t) {
        const size_t want = sizeof h + (off[F] - sizeof h) * t / nt;
        while (f < F && off[f] < want) ++f;
        fcut[t] = (uint32_t)f;
    }
    std::vector<uint64_t> bad(nt, UINT64_MAX);  // the feature row of a case id past the targets
    parallel_for(nt, [&](size_t t) {
        for (uint32_t f = fcut[t]; f < fcut[t + 1]; ++f) {
            uint32_t sz;
            std::memcpy(&sz, xb + off[f], 4);
            const char* rec = xb + off[f] + 4;
            for (uint32_t k = 0; k < sz; ++k, rec += 8) {
                uint32_t c;
                std::memcpy(&c, rec, 4);
                if (c >= C) {
                    bad[t] = f;
                    return;
                }
                const uint32_t slot = cnt[c].fetch_add(1, std::memory_order_relaxed);
                if (slot == 0) out->user[c] = f;
                else if (slot == 1) out->item[c] = f;
            }
        }
    });
    for (uint64_t f : bad)
        if (f != UINT64_MAX) {
            sbmf_free_ratings(out);
            return fail(xf + " feature row " + std::to_string(f) + ": case id past the " + std::to_string(C) + " targets");
        }
    std::vector<uint64_t> first_bad(nc, UINT64_MAX);
    parallel_for(nc, [&](size_t t) {
        for (size_t c = C * t / nc, e = C * (t + 1) / nc; c < e; ++c) {
            const uint32_t a = out->user[c], b2 = out->item[c];
            const uint32_t lo = std::min(a, b2), hi = std::max(a, b2);
            if (cnt[c].load(std::memory_order_relaxed) != 2 || hi < item_offset ||
                (item_offset > 0 && lo >= item_offset)) {
                first_bad[t] = c;
                return;
            }
            out->user[c] = lo;
            out->item[c] = hi - item_offset;
            out->rating[c] = (double)b.target(c);
        }
    });
    for (uint64_t c : first_bad)
        if (c != UINT64_MAX) {
            sbmf_free_ratings(out);
            return fail(xf + " case " + std::to_string(c) + ": the learners need exactly one user and one item feature "
                        "per case (" + std::to_string(cnt[c].load()) + " features" +
                        (item_offset > 0 ? "; user id < item_offset <= item id)" : ")") +
                        "; cases with any other number of features are read from libFM text only (sbmf_load_libfm_cases)");
        }
    out->n = C;
    return SBMF_OK;
}

// the first of Data::load's two pairs of names with both files present, loaded
int load_pair(const char* stem, bool transposed, uint32_t item_offset, sbmf_ratings* out) {
    if (!stem || !out) return SBMF_E_ARG;
    std::memset(out, 0, sizeof *out);
    const std::string s(stem);
    for (const Names& nm : NAMES)
        if (file_exists(s + nm.matrix(transposed)) && file_exists(s + nm.y))
            return (transposed ? load_xt : load_x)(s + nm.matrix(transposed), s + nm.y, item_offset, out);
    return fail("unable to open " + s + OWN.matrix(transposed) + "/" + OWN.y + " (or " + NAMES[0].matrix(transposed) + "/" +
                NAMES[0].y + ")");
}

// ---- libFM's block-structure relations (relation.h): <stem>.xt or <stem>.x (the block table as a
// binary sparse matrix, the layout above), <stem>.train / <stem>.test (the block row of every case:
// text, one unsigned integer per case, or a binary DVector<uint>: u32 version = 1; u32 size = 4;
// u32 dim; dim x u32 -- RelationJoin::load, relation.h:65-88) and the optional <stem>.groups.

// a binary sparse matrix as rows of {id, value}: ptr[num_rows + 1], ids, values
int read_fmatrix(const std::string& path, FmHeader& h, std::vector<uint64_t>& ptr, std::vector<uint32_t>& id,
                 std::vector<float>& val) {
    InFile in;
    if (const int rc = open_or_fail(path, in)) return rc;
    if (const int rc = matrix_header(path, in, h)) return rc;
    ptr.assign(1, 0);
    id.clear();
    val.clear();
    uint64_t nv;
    const bool whole = walk_rows(path, in, h.num_rows, "row", nv, [&](uint32_t r, size_t at, uint32_t sz) {
        for (uint32_t k = 0; k < sz; ++k) {
            uint32_t a;
            float v;
            std::memcpy(&a, in.p + at + 4 + 8 * (size_t)k, 4);
            std::memcpy(&v, in.p + at + 8 + 8 * (size_t)k, 4);
            if (a >= h.num_cols)
                return fail(path + " row " + std::to_string(r) + ": entry " + std::to_string(k) + " has id " +
                            std::to_string(a) + "; the file has " + std::to_string(h.num_cols) + " columns"), false;
            id.push_back(a);
            val.push_back(v);
        }
        ptr.push_back(id.size());
        return true;
    });
    if (!whole) return SBMF_E_IO;
    if (nv != h.num_values)
        return fail(path + ": " + std::to_string(nv) + " entries read, the header says " + std::to_string(h.num_values));
    return SBMF_OK;
}

// the block row of every case, in either form
int read_row_map(const std::string& path, uint32_t** out, uint64_t* n) {
    *out = nullptr;
    *n = 0;
    InFile in;
    if (const int rc = open_or_fail(path, in)) return rc;
    std::vector<uint32_t> v;
    uint32_t hd[3] = {0, 0, 0};
    if (in.n >= 8) std::memcpy(hd, in.p, in.n >= 12 ? 12 : 8);
    if (in.n >= 8 && hd[0] == 1 && hd[1] == sizeof(uint32_t)) {  // RelationJoin::load's test for the binary form
        if (in.n < 12 || in.n < 12 + (size_t)hd[2] * 4)
            return fail(path + ": a binary DVector<uint> of " + std::to_string(hd[2]) + " entries, truncated");
        v.resize(hd[2]);
        if (hd[2]) std::memcpy(v.data(), in.p + 12, (size_t)hd[2] * 4);
    } else {
        const char* q = in.p;
        uint32_t x;
        while (const int got = next_uint(q, in.p + in.n, x)) {
            if (got < 0)
                return fail(path + ": entry " + std::to_string(v.size() + 1) + " is not a block-row index (an unsigned integer)");
            v.push_back(x);
        }
    }
    *out = static_cast<uint32_t*>(std::malloc(std::max<size_t>(v.size(), 1) * sizeof(uint32_t)));
    if (!*out) return SBMF_E_NOMEM;
    std::copy(v.begin(), v.end(), *out);
    *n = v.size();
    return SBMF_OK;
}

// ---- the writers' shared parts

void write_matrix_header(OutFile& f, uint64_t num_values, uint64_t num_rows, uint64_t num_cols) {
    const FmHeader h{2, (uint32_t)sizeof(float), num_values, (uint32_t)num_rows, (uint32_t)num_cols};
    f.write(&h, sizeof h);
}

// one row {u32 size; size x {u32 id; f32 value}} in one write: id(k), value(k) give its k-th entry
template <class I, class V>
void write_row(OutFile& f, std::vector<char>& buf, uint32_t sz, I&& id, V&& value) {
    buf.resize(4 + (size_t)sz * 8);
    std::memcpy(buf.data(), &sz, 4);
    for (uint32_t k = 0; k < sz; ++k) {
        const uint32_t a = id(k);
        const float v = value(k);
        std::memcpy(buf.data() + 4 + 8 * (size_t)k, &a, 4);
        std::memcpy(buf.data() + 8 + 8 * (size_t)k, &v, 4);
    }
    f.write(buf.data(), buf.size());
}

// the target file of n ratings: the header, then the ratings as f32
void write_targets(OutFile& f, const double* rating, uint64_t n) {
    const uint32_t h[3] = {1, (uint32_t)sizeof(float), (uint32_t)n};
    f.write(h, sizeof h);
    constexpr size_t CH = 1 << 16;  // values per buffered write
    std::vector<float> buf(CH);
    for (uint64_t q0 = 0; f.ok() && q0 < n; q0 += CH) {
        const size_t m = (size_t)std::min<uint64_t>(CH, n - q0);
        for (size_t k = 0; k < m; ++k) buf[k] = (float)rating[q0 + k];
        f.write(buf.data(), 4 * m);
    }
}

// The two rating writers' arguments, and their num_cols = max(num_cols, largest feature id + 1).
// Feature ids are written as uint32 and num_cols must fit too: computed in 64 bits, anything past
// UINT32_MAX - 1 is refused (no wrap).
int rating_cols(const char* stem, const sbmf_ratings* in, uint32_t item_offset, uint32_t num_cols, const char* ext,
                uint64_t& cols) {
    if (!stem || !in || (in->n && (!in->user || !in->item || !in->rating))) return SBMF_E_ARG;
    if (in->n > 0xffffffffull) return SBMF_E_ARG;
    cols = num_cols;
    for (uint64_t q = 0; q < in->n; ++q) {
        cols = std::max<uint64_t>(cols, (uint64_t)in->user[q] + 1);
        cols = std::max<uint64_t>(cols, (uint64_t)item_offset + in->item[q] + 1);
    }
    if (cols > 0xffffffffull)
        return fail(std::string("feature id past UINT32_MAX - 1 (item_offset + item id): not representable in the ") + ext +
                        " format",
                    SBMF_E_ARG);
    return SBMF_OK;
}

// <stem><ext> and <stem>.y opened for a rating writer's `body`, the targets written after it
template <class Body>
int save_pair(const char* stem, const char* ext, const sbmf_ratings* in, Body&& body) {
    const std::string s(stem), both = s + ext + "/" + OWN.y;
    OutFile fx(s + ext), fy;
    if (!fx.ok() || !fy.open(s + OWN.y)) return fail("unable to write " + both);
    body(fx);
    if (fx.ok()) write_targets(fy, in->rating, in->n);
    const bool x_ok = fx.close(), y_ok = fy.close();
    if (!x_ok || !y_ok) return fail("write error on " + both);
    return SBMF_OK;
}

}  // namespace

extern "C" {

const char* sbmf_loader_error(void) { return g_lerr.c_str(); }

void sbmf_free_ratings(sbmf_ratings* r) {
    if (!r) return;
    std::free(r->user);
    std::free(r->item);
    std::free(r->rating);
    r->user = r->item = nullptr;
    r->rating = nullptr;
    r->n = 0;
}

void sbmf_free_cases(sbmf_cases* c) {
    if (!c) return;
    std::free(c->ptr);
    std::free(c->attr);
    std::free(c->x);
    std::free(c->target);
    std::memset(c, 0, sizeof *c);
}

void sbmf_free_relation(sbmf_cases* block, uint32_t** train_row, uint32_t** test_row, uint32_t** group) {
    sbmf_free_cases(block);
    for (uint32_t** p : {train_row, test_row, group})
        if (p) {
            std::free(*p);
            *p = nullptr;
        }
}

int sbmf_load_triples(const char* path, sbmf_ratings* out) {
    if (!path || !out) return SBMF_E_ARG;
    std::memset(out, 0, sizeof *out);
    InFile f;
    if (const int rc = open_or_fail(path, f)) return rc;
    return run_chunks(f.p, f.n, path, [](Part& P, const char* p, const char* e) {
        walk_lines(P, p, e, [&P](const char* a, const char* le) { return triple_fast(P, a, le); },
                   [&P](const char* t) { return triple_slow(P, t); });
    }, out);
}

int sbmf_load_libfm(const char* path, uint32_t item_offset, sbmf_ratings* out) {
    if (!path || !out) return SBMF_E_ARG;
    std::memset(out, 0, sizeof *out);
    InFile f;
    if (const int rc = open_or_fail(path, f)) return rc;
    return run_chunks(f.p, f.n, path, [item_offset](Part& P, const char* p, const char* e) {
        parse_libfm(RatingSink{P, item_offset}, p, e);
    }, out);
}

// The same line-aligned chunks on threads as run_chunks, concatenated in file order.
int sbmf_load_libfm_cases(const char* path, sbmf_cases* out) {
    if (!path || !out) return SBMF_E_ARG;
    std::memset(out, 0, sizeof *out);
    InFile f;
    if (const int rc = open_or_fail(path, f)) return rc;
    const std::vector<size_t> cut = text_chunks(f.p, f.n);
    const size_t nc = cut.size() - 1;
    std::vector<CasePart> parts(nc);
    parallel_for(nc, [&](size_t c) {
        CasePart P;  // as run_chunks' parts
        parse_libfm(CaseSink{P}, f.p + cut[c], f.p + cut[c + 1]);
        parts[c] = std::move(P);
    });
    if (const int rc = first_error(parts, path)) return rc;
    size_t n = 0, nnz = 0;
    uint32_t mx = 0;
    bool any = false;
    for (const CasePart& p : parts) {
        n += p.len.size();
        nnz += p.attr.size();
        mx = std::max(mx, p.max_attr);
        any = any || p.any;
    }
    out->ptr = static_cast<uint64_t*>(big_alloc((n + 1) * sizeof(uint64_t)));
    out->attr = static_cast<uint32_t*>(big_alloc(std::max<size_t>(nnz, 1) * sizeof(uint32_t)));
    out->x = static_cast<float*>(big_alloc(std::max<size_t>(nnz, 1) * sizeof(float)));
    out->target = static_cast<float*>(big_alloc(std::max<size_t>(n, 1) * sizeof(float)));
    if (!out->ptr || !out->attr || !out->x || !out->target) {
        sbmf_free_cases(out);
        return SBMF_E_NOMEM;
    }
    std::vector<size_t> c0(nc + 1, 0), e0(nc + 1, 0);
    for (size_t c = 0; c < nc; ++c) {
        c0[c + 1] = c0[c] + parts[c].len.size();
        e0[c + 1] = e0[c] + parts[c].attr.size();
    }
    parallel_for(nc, [&](size_t c) {
        const CasePart& p = parts[c];
        uint64_t at = e0[c];
        for (size_t k = 0; k < p.len.size(); ++k) {
            out->ptr[c0[c] + k] = at;
            at += p.len[k];
        }
        if (!p.attr.empty()) {
            std::memcpy(out->attr + e0[c], p.attr.data(), p.attr.size() * sizeof(uint32_t));
            std::memcpy(out->x + e0[c], p.x.data(), p.x.size() * sizeof(float));
        }
        if (!p.y.empty()) std::memcpy(out->target + c0[c], p.y.data(), p.y.size() * sizeof(float));
    });
    out->ptr[n] = nnz;
    out->n = n;
    out->nnz = nnz;
    out->num_attr = any ? mx + 1 : 0;
    return SBMF_OK;
}

int sbmf_load_libfm_binary(const char* stem, uint32_t item_offset, sbmf_ratings* out) {
    return load_pair(stem, false, item_offset, out);
}

int sbmf_load_libfm_binary_t(const char* stem, uint32_t item_offset, sbmf_ratings* out) {
    return load_pair(stem, true, item_offset, out);
}

// Data::load's file choice (Data.h:112-117): 1 = <stem>.data/.datat/.target,
// 2 = <stem>.x/.xt/.y, each file of the pair required only when the data set
// needs that orientation (has_x: row-major cases; has_xt: the transpose, rows
// per feature), 0 = neither, Data::load reads <stem> as text.  bin/libFM builds
// its train / test sets with has_x = (method != "mcmc") after rewriting als to
// mcmc, and has_xt = true except for sgd / sgda (libfm.cpp:132-149): the MCMC
// and ALS chains read only the transpose.
int sbmf_libfm_binary_kind(const char* stem, int has_x, int has_xt) {
    if (!stem || (!has_x && !has_xt)) return SBMF_E_ARG;
    const std::string s(stem);
    for (int k = 0; k < 2; ++k)
        if ((!has_x || file_exists(s + NAMES[k].x)) && (!has_xt || file_exists(s + NAMES[k].xt)) &&
            file_exists(s + NAMES[k].y))
            return k + 1;
    return 0;
}

// Data::load (Data.h:106-283) for rating data: the binary files of
// sbmf_libfm_binary_kind when present (the row-major file when the set has one;
// the transpose for a set without, which is what bin/libFM's MCMC / ALS sets
// read), else <stem> as libFM text.
int sbmf_load_libfm_data(const char* stem, int has_x, int has_xt, uint32_t item_offset, sbmf_ratings* out) {
    if (!stem || !out || (!has_x && !has_xt)) return SBMF_E_ARG;
    std::memset(out, 0, sizeof *out);
    const int kind = sbmf_libfm_binary_kind(stem, has_x, has_xt);
    if (kind == 0) return sbmf_load_libfm(stem, item_offset, out);
    const Names& nm = NAMES[kind - 1];
    const std::string s(stem);
    return (has_x ? load_x : load_xt)(s + nm.matrix(!has_x), s + nm.y, item_offset, out);
}

// DataMetaInfo::loadGroupsFromFile (Data.h:49-61): DVector<uint>::load reads num_attr values with
// operator>>.  Where that reads past the end or meets something that is no number (and goes on
// with what it has), this refuses, naming the entry.
int sbmf_load_libfm_meta(const char* path, uint32_t num_attr, uint32_t* group, uint32_t* G) {
    if (!path || (num_attr && !group)) return SBMF_E_ARG;
    InFile f;
    if (const int rc = open_or_fail(path, f)) return rc;
    const char* q = f.p;
    uint32_t mx = 0;
    for (uint32_t a = 0; a < num_attr; ++a) {
        const int got = next_uint(q, f.p + f.n, group[a]);
        if (got == 0)
            return fail(std::string(path) + " holds " + std::to_string(a) + " group ids; " + std::to_string(num_attr) +
                        " attributes need one each (entry " + std::to_string(a + 1) + " is missing)");
        if (got < 0)
            return fail(std::string(path) + ": entry " + std::to_string(a + 1) + " is not a group id (an unsigned integer)");
        mx = std::max(mx, group[a]);
    }
    if (G) *G = num_attr ? mx + 1 : 0;
    return SBMF_OK;
}

int sbmf_load_libfm_relation(const char* stem, sbmf_cases* block, uint32_t** train_row, uint64_t* n_train,
                             uint32_t** test_row, uint64_t* n_test, uint32_t** group, uint32_t* G) {
    if (!stem || !block || !train_row || !n_train || !test_row || !n_test || !group || !G) return SBMF_E_ARG;
    std::memset(block, 0, sizeof *block);
    *train_row = *test_row = *group = nullptr;
    *n_train = *n_test = 0;
    *G = 0;
    const std::string s(stem);
    FmHeader h{};
    std::vector<uint64_t> ptr;
    std::vector<uint32_t> id;
    std::vector<float> val;
    const bool t = file_exists(s + OWN.xt);
    if (!t && !file_exists(s + OWN.x)) return fail("unable to open " + s + OWN.xt + " (or " + OWN.x + ")");
    int rc = read_fmatrix(s + OWN.matrix(t), h, ptr, id, val);
    if (rc != SBMF_OK) return rc;
    // .xt: a row is an attribute and its entries the block rows holding it, ascending
    const uint32_t nb = t ? h.num_cols : h.num_rows, pa = t ? h.num_rows : h.num_cols;
    const size_t nnz = id.size();
    block->n = nb;
    block->nnz = nnz;
    block->num_attr = pa;
    block->ptr = static_cast<uint64_t*>(std::calloc((size_t)nb + 1, sizeof(uint64_t)));
    block->attr = static_cast<uint32_t*>(std::malloc(std::max<size_t>(nnz, 1) * sizeof(uint32_t)));
    block->x = static_cast<float*>(std::malloc(std::max<size_t>(nnz, 1) * sizeof(float)));
    block->target = static_cast<float*>(std::calloc(std::max<size_t>(nb, 1), sizeof(float)));
    auto bail = [&](int code) {
        sbmf_free_relation(block, train_row, test_row, group);
        return code;
    };
    if (!block->ptr || !block->attr || !block->x || !block->target) return bail(SBMF_E_NOMEM);
    if (t) {
        for (size_t k = 0; k < nnz; ++k) block->ptr[id[k] + 1]++;
        for (uint32_t j = 0; j < nb; ++j) block->ptr[j + 1] += block->ptr[j];
        std::vector<uint64_t> fill(block->ptr, block->ptr + nb);
        for (uint32_t a = 0; a < pa; ++a)
            for (uint64_t k = ptr[a]; k < ptr[a + 1]; ++k) {
                const uint64_t at = fill[id[k]]++;
                block->attr[at] = a;
                block->x[at] = val[k];
            }
    } else {
        std::copy(ptr.begin(), ptr.end(), block->ptr);
        std::copy(id.begin(), id.end(), block->attr);
        std::copy(val.begin(), val.end(), block->x);
    }
    if ((rc = read_row_map(s + ".train", train_row, n_train)) != SBMF_OK) return bail(rc);
    if ((rc = read_row_map(s + ".test", test_row, n_test)) != SBMF_OK) return bail(rc);
    if (file_exists(s + ".groups")) {
        *group = static_cast<uint32_t*>(std::malloc(std::max<size_t>(pa, 1) * sizeof(uint32_t)));
        if (!*group) return bail(SBMF_E_NOMEM);
        if ((rc = sbmf_load_libfm_meta((s + ".groups").c_str(), pa, *group, G)) != SBMF_OK) return bail(rc);
    }
    return SBMF_OK;
}

// The SBPMF triple format the reference's data scripts write
// (data/*/create_file_scalable_bpmf.py: "u\ti\tr" per line, 0-based ids),
// ratings printed with %.17g unless they are integers (as "4", "3.5" in
// MovieLens), so sbmf_load_triples reads back the same doubles.
int sbmf_save_triples(const char* path, const sbmf_ratings* in) {
    if (!path || !in || (in->n && (!in->user || !in->item || !in->rating))) return SBMF_E_ARG;
    OutFile f(path);
    if (!f.ok()) return fail(std::string("unable to write ") + path);
    auto put_u = [](char* o, unsigned long long v) {  // decimal digits of v at o, returns the end
        char t[24];
        int k = 0;
        do {
            t[k++] = (char)('0' + v % 10);
            v /= 10;
        } while (v);
        while (k) *o++ = t[--k];
        return o;
    };
    std::vector<char> buf(1 << 22);
    size_t at = 0;
    for (uint64_t q = 0; f.ok() && q < in->n; ++q) {
        if (at + 96 > buf.size()) {
            f.write(buf.data(), at);
            at = 0;
        }
        char* o = buf.data() + at;
        o = put_u(o, in->user[q]);
        *o++ = '\t';
        o = put_u(o, in->item[q]);
        *o++ = '\t';
        const double r = in->rating[q];
        if (r >= 0 && r < 1e15 && r == (double)(long long)r && !std::signbit(r))
            o = put_u(o, (unsigned long long)r);
        else
            o += std::snprintf(o, 40, "%.17g", r);
        *o++ = '\n';
        at = (size_t)(o - buf.data());
    }
    f.write(buf.data(), at);
    if (!f.close()) return fail(std::string("write error on ") + path);
    return SBMF_OK;
}

// the convert tool's output for rating data (tools/convert.cpp:55-205): row q
// holds {user[q]:1, item_offset + item[q]:1}, target rating[q] as f32
int sbmf_save_libfm_binary(const char* stem, const sbmf_ratings* in, uint32_t item_offset, uint32_t num_cols) {
    uint64_t cols;
    if (const int rc = rating_cols(stem, in, item_offset, num_cols, OWN.x, cols)) return rc;
    return save_pair(stem, OWN.x, in, [&](OutFile& fx) {
        write_matrix_header(fx, 2 * in->n, in->n, cols);
        constexpr size_t CH = 1 << 16;  // rows per buffered write
        std::vector<char> xb(CH * 20);
        for (uint64_t q0 = 0; fx.ok() && q0 < in->n; q0 += CH) {
            const size_t m = (size_t)std::min<uint64_t>(CH, in->n - q0);
            for (size_t k = 0; k < m; ++k) {
                const uint64_t q = q0 + k;
                const uint32_t sz = 2, a = in->user[q], b = item_offset + in->item[q];
                const float one = 1.0f;
                char* row = xb.data() + k * 20;
                std::memcpy(row, &sz, 4);
                std::memcpy(row + 4, &a, 4);
                std::memcpy(row + 8, &one, 4);
                std::memcpy(row + 12, &b, 4);
                std::memcpy(row + 16, &one, 4);
            }
            fx.write(xb.data(), 20 * m);
        }
    });
}

// tools/transpose.cpp:54-172 for rating data: <stem>.xt holds one row per
// feature 0..num_cols-1 (num_cols = max(num_cols, largest feature id + 1), as
// the .x writer), each the ascending case ids of that feature with value 1, and
// <stem>.y the f32 targets -- byte for byte what convert + transpose write for
// the same cases (a .x row {user, item} with value 1 each).
int sbmf_save_libfm_binary_t(const char* stem, const sbmf_ratings* in, uint32_t item_offset, uint32_t num_cols) {
    uint64_t cols;
    if (const int rc = rating_cols(stem, in, item_offset, num_cols, OWN.xt, cols)) return rc;
    for (uint64_t q = 0; q < in->n; ++q)
        if (in->user[q] == (uint64_t)item_offset + in->item[q])
            return fail("case " + std::to_string(q) + ": user and item feature ids coincide", SBMF_E_ARG);
    // counting sort of the 2n (feature, case) entries by feature, cases ascending
    std::vector<uint64_t> start(cols + 1, 0);
    for (uint64_t q = 0; q < in->n; ++q) {
        ++start[in->user[q] + 1];
        ++start[(uint64_t)item_offset + in->item[q] + 1];
    }
    for (uint64_t f = 0; f < cols; ++f) start[f + 1] += start[f];
    std::vector<uint32_t> cs(2 * in->n);
    {
        std::vector<uint64_t> fill(start.begin(), start.end() - 1);
        for (uint64_t q = 0; q < in->n; ++q) {
            cs[fill[in->user[q]]++] = (uint32_t)q;
            cs[fill[(uint64_t)item_offset + in->item[q]]++] = (uint32_t)q;
        }
    }
    return save_pair(stem, OWN.xt, in, [&](OutFile& fx) {
        write_matrix_header(fx, 2 * in->n, cols, in->n);
        std::vector<char> buf;
        for (uint64_t f = 0; fx.ok() && f < cols; ++f)
            write_row(fx, buf, (uint32_t)(start[f + 1] - start[f]), [&](uint32_t k) { return cs[start[f] + k]; },
                      [](uint32_t) { return 1.0f; });
    });
}

int sbmf_save_libfm_block(const char* path, const sbmf_cases* block) {
    if (!path || !block || (block->n && !block->ptr) || (block->nnz && (!block->attr || !block->x))) return SBMF_E_ARG;
    OutFile f(path);
    if (!f.ok()) return fail(std::string("unable to open ") + path + " for writing");
    write_matrix_header(f, block->nnz, block->n, block->num_attr);
    std::vector<char> buf;
    for (uint64_t j = 0; j < block->n && f.ok(); ++j) {
        const uint64_t k0 = block->ptr[j];
        write_row(f, buf, (uint32_t)(block->ptr[j + 1] - k0), [&](uint32_t k) { return block->attr[k0 + k]; },
                  [&](uint32_t k) { return block->x[k0 + k]; });
    }
    if (!f.close()) return fail(std::string("write error on ") + path);
    return SBMF_OK;
}

int sbmf_save_libfm_row_map(const char* path, const uint32_t* row, uint64_t n, int binary) {
    if (!path || (n && !row) || n > 0xffffffffull) return SBMF_E_ARG;
    OutFile f(path);
    if (!f.ok()) return fail(std::string("unable to open ") + path + " for writing");
    if (binary) {
        const uint32_t hd[3] = {1, (uint32_t)sizeof(uint32_t), (uint32_t)n};
        f.write(hd, sizeof hd);
        f.write(row, 4 * (size_t)n);
    } else {
        char line[16];
        for (uint64_t c = 0; c < n && f.ok(); ++c) f.write(line, (size_t)std::snprintf(line, sizeof line, "%u\n", row[c]));
    }
    if (!f.close()) return fail(std::string("write error on ") + path);
    return SBMF_OK;
}

}  // extern "C"
