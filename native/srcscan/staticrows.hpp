// Class / method rows of a scan, built natively for the bulk writer: the
// UUIDv7 generator, the row builder and the emitter that turns ranges of a
// ScanResult's files into INSERT batches.  No Python here: the emitter runs
// on scan worker threads without the GIL (pymodule.cpp), and a stand-alone
// program can drive it (stream_rows_check.cpp).
#pragma once

#include <sys/random.h>

#include <algorithm>
#include <cctype>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <deque>
#include <exception>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <thread>
#include <utility>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "bulkwriter.hpp"
#include "srcscan.hpp"

namespace staticrows {

// One INSERT's rows, appended value by value (text values are views).
struct TextRows {
    dbw::Batch b;
    explicit TextRows(const std::string& sql, int ncols) {
        b.sql = sql;
        b.ncols = ncols;
    }
    void null() { b.values.emplace_back(); }
    void text(const char* p, size_t n) {
        dbw::Value v;
        v.kind = dbw::Value::Text;
        v.p = p;
        v.n = static_cast<int32_t>(n);
        b.values.push_back(v);
    }
    void owned(std::string&& s) {
        b.owned.push_back(std::move(s));
        text(b.owned.back().data(), b.owned.back().size());
    }
    void integer(long long i) {
        dbw::Value v;
        v.kind = dbw::Value::Int;
        v.i = i;
        b.values.push_back(v);
    }
    bool empty() const { return b.values.empty(); }
};

// Time-ordered version-7 UUID strings (RFC 9562): 48-bit ms timestamp, then
// a 74-bit counter started at a random point (rand_a + rand_b), so a batch is
// strictly increasing and bulk inserts append to the primary-key B-trees.
struct Uuid7Gen {
    unsigned long long ms = 0, hi = 0, lo = 0;
    Uuid7Gen() {
        unsigned char seed[10];
        if (getrandom(seed, sizeof(seed), 0) != (ssize_t)sizeof(seed)) throw std::runtime_error("getrandom failed");
        ms = (unsigned long long)std::chrono::duration_cast<std::chrono::milliseconds>(
                 std::chrono::system_clock::now().time_since_epoch())
                 .count();
        // counter: 12 bits (rand_a) + 62 bits (rand_b); start in the lower half to avoid overflow
        hi = ((unsigned long long)(seed[0] & 0x07) << 8) | seed[1];  // 11 bits
        for (int j = 2; j < 10; ++j) lo = (lo << 8) | seed[j];
        lo &= 0x1FFFFFFFFFFFFFFFull;  // 61 bits
    }
    void next(char* s) {  // 36 chars
        static const char* hex = "0123456789abcdef";
        unsigned char b[16];
        for (int j = 0; j < 6; ++j) b[j] = (unsigned char)(ms >> (8 * (5 - j)));
        b[6] = (unsigned char)(0x70 | ((hi >> 8) & 0x0F));
        b[7] = (unsigned char)(hi & 0xFF);
        b[8] = (unsigned char)(0x80 | ((lo >> 56) & 0x3F));
        for (int j = 9; j < 16; ++j) b[j] = (unsigned char)(lo >> (8 * (15 - j)));
        if (++lo >> 62) {
            lo = 0;
            ++hi;
        }
        int k = 0;
        for (int j = 0; j < 16; ++j) {
            if (j == 4 || j == 6 || j == 8 || j == 10) s[k++] = '-';
            s[k++] = hex[b[j] >> 4];
            s[k++] = hex[b[j] & 15];
        }
    }
};

// json.dumps(list_of_str) (default separators, ensure_ascii) of UTF-8 strings
inline void json_ascii_list(const std::vector<std::string>& v, std::string& out) {
    static const char* hex = "0123456789abcdef";
    auto u4 = [&](unsigned c) {
        out += "\\u";
        for (int sh = 12; sh >= 0; sh -= 4) out += hex[(c >> sh) & 15];
    };
    out = "[";
    for (size_t i = 0; i < v.size(); ++i) {
        if (i) out += ", ";
        out += '"';
        const std::string& s = v[i];
        for (size_t k = 0; k < s.size();) {
            unsigned char c = (unsigned char)s[k];
            unsigned cp = c;
            size_t len = 1;
            if (c >= 0xF0 && k + 3 < s.size() + 0) { cp = ((c & 7u) << 18) | ((s[k + 1] & 63u) << 12) | ((s[k + 2] & 63u) << 6) | (s[k + 3] & 63u); len = 4; }
            else if (c >= 0xE0 && k + 2 < s.size()) { cp = ((c & 15u) << 12) | ((s[k + 1] & 63u) << 6) | (s[k + 2] & 63u); len = 3; }
            else if (c >= 0xC0 && k + 1 < s.size()) { cp = ((c & 31u) << 6) | (s[k + 1] & 63u); len = 2; }
            k += len;
            if (cp == '"') out += "\\\"";
            else if (cp == '\\') out += "\\\\";
            else if (cp == '\n') out += "\\n";
            else if (cp == '\r') out += "\\r";
            else if (cp == '\t') out += "\\t";
            else if (cp == '\b') out += "\\b";
            else if (cp == '\f') out += "\\f";
            else if (cp < 0x20 || (cp >= 0x7f && cp < 0x10000)) u4(cp);
            else if (cp >= 0x10000) {
                cp -= 0x10000;
                u4(0xD800 + (cp >> 10));
                u4(0xDC00 + (cp & 0x3FF));
            } else out += (char)cp;
        }
        out += '"';
    }
    out += "]";
}

// Class and method rows of a scan handed to the bulk writer before any
// Python object exists -- for Java while the scan is still parsing later
// files -- so the inserts start while the caller still builds the graph;
// Phase 1 then only binds the ids (phase1_rows with pre_ids) and writes the
// parameter rows.  Java / TypeScript units (a later file with the same
// identifier replaces the earlier one, as parsers/base.py::_add_unit does);
// Go merges files per package: not here.
// The rows view the ScanResult's strings and the id blocks, which the
// batches keep alive (freed off the writer thread after the inserts).
struct StaticRowsSpec {
    dbw::BulkWriter* writer = nullptr;
    std::string pid, now, commit, cls_sql, meth_sql;
    bool commit_null = false;
};

struct StaticRowsKeep {
    std::shared_ptr<const srcscan::ScanResult> r;
    StaticRowsSpec spec;
    // 36 chars per id: per emitted file its class id, then its method ids,
    // contiguous.  Fixed blocks that are never reallocated or moved: rows
    // already handed to the writer view them while later ids are generated.
    std::vector<std::unique_ptr<char[]>> id_blocks;
    std::vector<const char*> first;   // per file: its class id in a block (nullptr: replaced file)
    std::deque<std::string> strings;  // JSON exception lists
};

inline const std::string& normalize_class_type(const std::string& t) {
    static const std::string kTypes[] = {"CONTROLLER", "SERVICE", "REPOSITORY", "ENTITY", "DTO",
                                         "CONFIGURATION", "LISTENER", "UTILITY", "EXCEPTION", "OTHER"};
    for (const std::string& k : kTypes) {
        if (k.size() != t.size()) continue;
        bool eq = true;
        for (size_t i = 0; i < t.size() && eq; ++i) eq = std::toupper((unsigned char)t[i]) == k[i];
        if (eq) return k;
    }
    return kTypes[9];  // ClassType.from_string: OTHER
}

// Rows of StaticRowsKeep::r's files, fed as ranges [a, b) in increasing
// order: all at once after the scan, or from the scan's row sink while later
// files are still parsed (then on the EmitterThread below; one caller at a time).
// GIL not needed and no Python object touched: reads the ScanResult -- only
// fields the resolution pass never writes (see FileRec) -- which a concurrent
// Python object build may read too.  Every file's identifier must be set
// before the first range: the last file of an identifier is the one emitted.
class StaticRowsEmitter {
public:
    explicit StaticRowsEmitter(std::shared_ptr<StaticRowsKeep> keep)
        : keep_(std::move(keep)), cls_(keep_->spec.cls_sql, 10), meth_(keep_->spec.meth_sql, 10) {}

    const std::shared_ptr<StaticRowsKeep>& keep() const { return keep_; }
    size_t fed() const { return next_; }
    size_t streamed = 0;  // files that arrived through the scan's sink
    bool finished() const { return finished_; }
    long long us() const { return us_; }

    void feed(const std::vector<srcscan::FileRec>& files, size_t a, size_t b) {
        const auto t = std::chrono::steady_clock::now();
        if (&files != &keep_->r->files || a != next_ || b > files.size() || finished_)
            throw std::logic_error("static rows: ranges must cover the scan's files in order");
        if (!started_) {
            started_ = true;
            last_.reserve(files.size() * 2);
            for (size_t k = 0; k < files.size(); ++k) last_[files[k].identifier] = k;
            keep_->first.assign(files.size(), nullptr);
        }
        for (size_t k = a; k < b; ++k) emit(files[k], k);
        next_ = b;
        us_ += since(t);
    }

    void finish() {  // the last partial chunk
        const auto t = std::chrono::steady_clock::now();
        flush(false);
        finished_ = true;
        us_ += since(t);
    }

private:
    static constexpr int kChunk = 256;           // classes per batch pair
    static constexpr size_t kIdBlock = 36 * 4096;

    static long long since(std::chrono::steady_clock::time_point t) {
        return std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t).count();
    }

    char* ids_for(size_t n) {  // room for n ids, contiguous
        const size_t need = 36 * n;
        if (need > block_left_) {
            block_left_ = std::max(need, kIdBlock);
            keep_->id_blocks.emplace_back(new char[block_left_]);
            block_at_ = keep_->id_blocks.back().get();
        }
        char* p = block_at_;
        block_at_ += need;
        block_left_ -= need;
        return p;
    }

    void flush(bool more) {
        const StaticRowsSpec& spec = keep_->spec;
        cls_.b.keep = keep_;
        meth_.b.keep = keep_;
        const size_t n_meth = meth_.b.values.size();
        if (!cls_.empty()) spec.writer->put(std::move(cls_.b));
        if (!meth_.empty()) spec.writer->put(std::move(meth_.b));
        cls_ = TextRows(spec.cls_sql, 10);
        meth_ = TextRows(spec.meth_sql, 10);
        if (more && n_meth) {  // the next chunk: no regrowth copies of a few hundred KB
            cls_.b.values.reserve(static_cast<size_t>(kChunk) * 10);
            meth_.b.values.reserve(n_meth + n_meth / 4);
        }
        pending_ = 0;
    }

    static void sv(TextRows& b, const std::string& s) { b.text(s.data(), s.size()); }

    void emit(const srcscan::FileRec& f, size_t k) {
        const StaticRowsSpec& spec = keep_->spec;
        if (last_[f.identifier] != k) return;
        if (pending_ == kChunk) flush(true);
        ++pending_;
        char* at = ids_for(1 + f.methods.size());
        keep_->first[k] = at;
        const char* cid = at;
        gen_.next(at);
        at += 36;
        const std::string& ident = f.identifier;
        const size_t dot = ident.rfind('.');
        TextRows& cls = cls_;
        TextRows& meth = meth_;
        cls.text(cid, 36);
        sv(cls, spec.pid);
        sv(cls, ident);
        if (dot != std::string::npos) cls.text(ident.data() + dot + 1, (ident.size() - dot - 1));
        else sv(cls, ident);
        if (dot != std::string::npos) cls.text(ident.data(), dot); else cls.null();
        sv(cls, normalize_class_type(f.class_type));
        cls.null();
        sv(cls, f.rel_path);
        sv(cls, spec.now);
        if (spec.commit_null) cls.null(); else sv(cls, spec.commit);
        for (const srcscan::MethodRec& m : f.methods) {
            gen_.next(at);
            meth.text(at, 36);
            at += 36;
            meth.text(cid, 36);
            sv(meth, m.name);
            meth.null();
            meth.text("[]", 2);
            if (m.exceptions.empty()) {
                meth.text("[]", 2);
            } else {
                keep_->strings.emplace_back();
                json_ascii_list(m.exceptions, keep_->strings.back());
                sv(meth, keep_->strings.back());
            }
            if (m.has_http_method) sv(meth, m.http_method); else meth.null();
            if (m.has_http_path) sv(meth, m.http_path); else meth.null();
            meth.integer(m.line);
            sv(meth, spec.now);
        }
    }

    std::shared_ptr<StaticRowsKeep> keep_;
    std::unordered_map<std::string_view, size_t> last_;
    Uuid7Gen gen_;
    TextRows cls_, meth_;
    int pending_ = 0;
    size_t next_ = 0;
    char* block_at_ = nullptr;
    size_t block_left_ = 0;
    bool started_ = false, finished_ = false;
    long long us_ = 0;
};

// The streamed emission's thread.  The scan's row sink only queues its range
// here (push), so no scan worker stops parsing to build rows: building a
// 2,000-class repository's rows on the workers lengthened the scan by 1.5-2 ms
// on the MI355X host, about what the earlier inserts won.  The thread feeds
// the emitter range by range -- one consumer, ranges in order -- and, once
// the queue is closed and every file went through it, hands over the last
// partial chunk.  close() before the ScanResult or the emitter goes away.
class EmitterThread {
public:
    explicit EmitterThread(StaticRowsEmitter& em) : em_(em), thread_([this] { run(); }) {}
    ~EmitterThread() { stop(); }
    EmitterThread(const EmitterThread&) = delete;
    EmitterThread& operator=(const EmitterThread&) = delete;

    void push(size_t a, size_t b) {  // the scan's sink (any worker thread)
        {
            std::lock_guard<std::mutex> g(mu_);
            ranges_.emplace_back(a, b);
        }
        cv_.notify_one();
    }

    void close() {  // no more ranges: waits for the emitter, rethrows what it threw
        stop();
        if (error_) std::rethrow_exception(error_);
    }

private:
    void stop() noexcept {
        if (!thread_.joinable()) return;
        {
            std::lock_guard<std::mutex> g(mu_);
            closed_ = true;
        }
        cv_.notify_one();
        thread_.join();
    }

    void run() noexcept {
        const std::vector<srcscan::FileRec>& files = em_.keep()->r->files;
        try {
            for (;;) {
                std::pair<size_t, size_t> r;
                {
                    std::unique_lock<std::mutex> lk(mu_);
                    cv_.wait(lk, [this] { return closed_ || !ranges_.empty(); });
                    if (ranges_.empty()) break;  // closed and drained
                    r = ranges_.front();
                    ranges_.pop_front();
                }
                em_.feed(files, r.first, r.second);
                em_.streamed += r.second - r.first;
            }
            // the scan is over (close() follows it): `files` is final
            if (em_.fed() == files.size()) em_.finish();
        } catch (...) {
            error_ = std::current_exception();
        }
    }

    StaticRowsEmitter& em_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<std::pair<size_t, size_t>> ranges_;
    bool closed_ = false;
    std::exception_ptr error_;
    std::thread thread_;  // last: started once the rest exists
};

// DMCP_STREAM_ROWS (default on; "0": off): a Java scan hands its rows to
// the writer while it parses, instead of after it.  Read per scan.
inline bool stream_rows_enabled() {
    const char* e = std::getenv("DMCP_STREAM_ROWS");
    return e == nullptr || e[0] != '0';
}

}  // namespace staticrows
