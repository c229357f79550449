// Stand-alone check of the streamed row emission (host only, no Python):
// mounts a generated Java tree, runs the scan with its row sink feeding a
// StaticRowsEmitter (on its EmitterThread, as the Python module does) into a
// BulkWriter on a temporary database file, commits,
// and verifies the rows; then does it again and rolls back after the rows
// were queued.  Meant for sanitizer builds of the real scan / emitter /
// writer code:
//
//   g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -o stream_rows_check stream_rows_check.cpp bulkwriter.cpp common.cpp java_frontend.cpp \
//       ts_frontend.cpp go_frontend.cpp project.cpp gitobj.cpp wire.cpp -l:libsqlite3.so.0 -lz
//   g++ -std=c++17 -O1 -g -pthread -fsanitize=thread \
//       -o stream_rows_check_tsan (the same sources and libraries)
//
// Usage: stream_rows_check [n_files=700] [threads=8]; exit status 0 = all checks passed.
#include <unistd.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "bulkwriter.hpp"
#include "sqlite_min.hpp"
#include "srcscan.hpp"
#include "staticrows.hpp"

namespace {

constexpr int OPEN_CREATE = 0x00000004;

const char* kSchema =
    "CREATE TABLE source_classes (id TEXT PRIMARY KEY, project_id TEXT NOT NULL, full_class_name TEXT NOT NULL,"
    " simple_name TEXT NOT NULL, package_name TEXT, class_type TEXT NOT NULL, description TEXT, source_file TEXT,"
    " created_at TEXT NOT NULL, commit_hash TEXT, UNIQUE(project_id, full_class_name));"
    "CREATE TABLE source_methods (id TEXT PRIMARY KEY, class_id TEXT NOT NULL, method_name TEXT NOT NULL,"
    " description TEXT, business_logic TEXT, exceptions TEXT, http_method TEXT, http_path TEXT,"
    " line_number INTEGER, created_at TEXT NOT NULL);"
    "CREATE INDEX idx_methods_class ON source_methods(class_id);";
const char* kClassSql = "INSERT INTO source_classes VALUES (?, ?, ?, ?, ?, ?, ?, ?, ?, ?)";
const char* kMethodSql = "INSERT INTO source_methods VALUES (?, ?, ?, ?, ?, ?, ?, ?, ?, ?)";

int failures = 0;
void check(bool ok, const char* what) {
    if (!ok) {
        std::fprintf(stderr, "FAILED: %s\n", what);
        ++failures;
    }
}

struct Db {
    sqlite3* db = nullptr;
    explicit Db(const std::string& path, int flags) {
        if (sqlite3_open_v2(path.c_str(), &db, flags, nullptr) != sqlite_min::OK) {
            std::fprintf(stderr, "cannot open %s\n", path.c_str());
            std::exit(2);
        }
    }
    ~Db() { sqlite3_close_v2(db); }
    void exec(const char* sql) {
        if (sqlite3_exec(db, sql, nullptr, nullptr, nullptr) != sqlite_min::OK) {
            std::fprintf(stderr, "%s: %s\n", sql, sqlite3_errmsg(db));
            std::exit(2);
        }
    }
    long long scalar(const char* sql) {
        long long v = -1;
        auto cb = [](void* out, int, char** cols, char**) {
            *static_cast<long long*>(out) = cols[0] ? std::atoll(cols[0]) : 0;
            return 0;
        };
        if (sqlite3_exec(db, sql, cb, &v, nullptr) != sqlite_min::OK) {
            std::fprintf(stderr, "%s: %s\n", sql, sqlite3_errmsg(db));
            std::exit(2);
        }
        return v;
    }
};

// n Java files, methods 0..4 per file, some with throws clauses and HTTP
// mappings; two paths that give the same identifier (the later one wins)
std::vector<std::pair<std::string, std::string>> java_tree(int n, long long& methods, long long& classes) {
    std::vector<std::pair<std::string, std::string>> tree;
    methods = 0;
    for (int k = 0; k < n; ++k) {
        const std::string name = "C" + std::to_string(k);
        std::string src = "package co.check.p" + std::to_string(k % 7) + ";\n\n";
        if (k % 3 == 0) src += "@org.springframework.web.bind.annotation.RestController\n";
        src += "public class " + name + " {\n";
        const int nm = k % 5;
        for (int j = 0; j < nm; ++j) {
            if (k % 3 == 0) src += "    @GetMapping(\"/c" + std::to_string(k) + "/m" + std::to_string(j) + "\")\n";
            src += "    public void m" + std::to_string(j) + "(String a)" +
                   (j % 2 ? " throws java.io.IOException, IllegalStateException" : "") + " {\n    }\n\n";
        }
        src += "}\n";
        methods += nm;
        tree.emplace_back("src/main/java/co/check/p" + std::to_string(k % 7) + "/" + name + ".java", std::move(src));
    }
    classes = n;
    if (n > 0) {  // identifier x.y.Twin twice: only x.y/Twin.java (walked last) is emitted
        tree.emplace_back("src/main/java/x/y/Twin.java", "package x.y;\npublic class Twin { void a() {} void b() {} }\n");
        tree.emplace_back("src/main/java/x.y/Twin.java", "package x.y;\npublic class Twin { void c() {} }\n");
        classes += 1;
        methods += 1;
    }
    tree.emplace_back("src/main/java/co/check/Broken.java", std::string("\xff\xfe{{{(\"\0class", 12));
    classes += 1;
    return tree;
}

// one scan of `tree` with the sink feeding an emitter into `writer`; returns files streamed
size_t scan_streaming(const std::vector<std::pair<std::string, std::string>>& tree, int threads,
                      dbw::BulkWriter& writer, size_t sink_chunk) {
    auto result = std::make_shared<srcscan::ScanResult>();
    auto keep = std::make_shared<staticrows::StaticRowsKeep>();
    keep->r = result;
    keep->spec.writer = &writer;
    keep->spec.pid = "project-1";
    keep->spec.now = "2024-01-01T00:00:00.000Z";
    keep->spec.commit_null = true;
    keep->spec.cls_sql = kClassSql;
    keep->spec.meth_sql = kMethodSql;
    staticrows::StaticRowsEmitter em(keep);
    keep.reset();  // from here the emitter and the queued batches own it
    staticrows::EmitterThread feeder(em);
    std::atomic<int> in_sink{0};
    srcscan::ScanOptions opt;
    opt.language = "java";
    opt.threads = threads;
    opt.sink_chunk = sink_chunk;
    size_t expect_first = 0;
    opt.file_sink = [&](const std::vector<srcscan::FileRec>& files, size_t a, size_t b) {
        check(in_sink.fetch_add(1) == 0, "sink calls never overlap");
        check(a == expect_first && a < b && b <= files.size(), "ranges are contiguous and increasing");
        expect_first = b;
        feeder.push(a, b);
        in_sink.fetch_sub(1);
    };
    auto copy = tree;
    const std::string root = srcscan::vfs_mount(std::move(copy));
    srcscan::scan_project_into(root, opt, *result);
    srcscan::vfs_unmount(root);
    check(expect_first == result->files.size(), "every file went through the sink before the scan returned");
    feeder.close();
    check(em.fed() == result->files.size() && em.finished(), "the emitter thread emitted every file");
    return em.streamed;
    // `result` and the emitter die here, before the writer has inserted all
    // batches: the batches' keep pointers hold what their rows view
}

}  // namespace

int main(int argc, char** argv) {
    const int n = argc > 1 ? std::atoi(argv[1]) : 700;
    const int threads = argc > 2 ? std::atoi(argv[2]) : 8;
    char path[] = "/tmp/stream_rows_check_XXXXXX";
    const int fd = mkstemp(path);
    if (fd < 0) return 2;
    close(fd);
    {
        Db db(path, sqlite_min::OPEN_READWRITE | OPEN_CREATE);
        db.exec(kSchema);
    }
    long long methods = 0, classes = 0;
    const auto tree = java_tree(n, methods, classes);
    {  // streamed rows, committed
        dbw::BulkWriter writer(path, 5000, {});
        const size_t streamed = scan_streaming(tree, threads, writer, 64);
        check(streamed == tree.size(), "all files streamed");
        writer.commit();
        const std::string err = writer.wait();
        check(err.empty(), "commit succeeded");
        check(writer.rows_written() == classes + methods, "rows written == classes + methods");
    }
    {
        Db db(path, sqlite_min::OPEN_READWRITE);
        check(db.scalar("SELECT COUNT(*) FROM source_classes") == classes, "class rows");
        check(db.scalar("SELECT COUNT(*) FROM source_methods") == methods, "method rows");
        check(db.scalar("SELECT COUNT(*) FROM source_methods m WHERE NOT EXISTS "
                        "(SELECT 1 FROM source_classes c WHERE c.id = m.class_id)") == 0, "methods point at classes");
        // ids ascend in insertion (= file) order
        check(db.scalar("SELECT COUNT(*) FROM (SELECT id, LAG(id) OVER (ORDER BY rowid) AS prev FROM source_classes) "
                        "WHERE prev IS NOT NULL AND prev >= id") == 0, "class ids ascend in file order");
        if (n > 0) {
            check(db.scalar("SELECT COUNT(*) FROM source_classes WHERE full_class_name = 'x.y.Twin' "
                            "AND source_file = 'src/main/java/x.y/Twin.java'") == 1, "the later twin wins");
            check(db.scalar("SELECT COUNT(*) FROM source_methods m JOIN source_classes c ON c.id = m.class_id "
                            "WHERE c.full_class_name = 'x.y.Twin'") == 1, "the later twin's methods only");
        }
    }
    {  // streamed rows (delivered file by file), then a rollback with batches still queued
        dbw::BulkWriter writer(path, 5000, {});
        for (const char* sql : {"DELETE FROM source_methods", "DELETE FROM source_classes"}) {
            dbw::Batch del;  // the old rows' deletes, as a re-analysis runs them
            del.sql = sql;
            writer.put(std::move(del));
        }
        scan_streaming(tree, threads, writer, 1);
        writer.abort();
        check(writer.wait() == "aborted", "abort reported");
    }
    {
        Db db(path, sqlite_min::OPEN_READWRITE);
        check(db.scalar("SELECT COUNT(*) FROM source_classes") == classes, "class rows after the rollback");
        check(db.scalar("SELECT COUNT(*) FROM source_methods") == methods, "method rows after the rollback");
    }
    unlink(path);
    std::printf("%s: %d files, %lld classes, %lld methods, %d threads\n", failures ? "FAILED" : "ok",
                (int)tree.size(), classes, methods, threads);
    return failures ? 1 : 0;
}
