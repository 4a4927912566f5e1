// Driver of tools/csv_bench.py: one CSV scan of `path` (columns i: Int64, f: Float64, b: Boolean, s: String) through
// the host CsvFileStream or the device reader (CsvScan::Device), every batch pulled, and the stages it is made of timed
// on their own: the file read into pinned memory and the upload of that many bytes.  Prints one JSON object.
//   csv_bench <path> <host|device|stages> <types, e.g. ifbs> [batch_rows]
#include <chrono>
#include <cstdio>
#include <fcntl.h>
#include <unistd.h>

#include "../rivulus_amd/host/rivulus_host.hpp"

using namespace rivulus;
using namespace rivulus::execution;

static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char **argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: csv_bench <path> <host|device|stages> <types> [batch_rows]\n");
        return 2;
    }
    const std::string path = argv[1], mode = argv[2], types = argv[3];
    const std::optional<size_t> batch = argc > 4 ? std::optional<size_t>(std::strtoull(argv[4], nullptr, 10)) : std::nullopt;
    std::vector<Field> f;
    for (char t : types)
        f.emplace_back(std::string(1, t) + std::to_string(f.size()),
                       t == 'i' ? DataType::Int64 : t == 'f' ? DataType::Float64 : t == 'b' ? DataType::Boolean : DataType::String, true);
    auto schema = std::make_shared<Schema>(f);
    auto ctx = std::make_shared<Context>(0);
    if (mode == "stages") {  // what the pipeline is made of: the file read (pinned, 64 MiB reads) and the upload of as many bytes
        const size_t chunk = 64u << 20;
        void *pinned = nullptr;
        check(rv_host_alloc(ctx->raw(), chunk, &pinned));
        const int fd = open(path.c_str(), O_RDONLY);
        double t0 = now();
        size_t total = 0;
        for (ssize_t k; (k = read(fd, pinned, chunk)) > 0;) total += static_cast<size_t>(k);
        const double read_s = now() - t0;
        close(fd);
        rv_column c{};
        c.dtype = RV_INT64;
        c.values = pinned;
        c.length = chunk / 8;
        t0 = now();
        for (size_t done = 0; done < total; done += chunk) {
            rv_dcolumn *d = nullptr;
            check(rv_upload(ctx->raw(), &c, &d));
            rv_free(ctx->raw(), d);
        }
        check(rv_ctx_synchronize(ctx->raw()));
        const double up_s = now() - t0;
        rv_host_free(ctx->raw(), pinned);
        std::printf("{\"bytes\": %zu, \"read_s\": %.4f, \"read_gbs\": %.3f, \"upload_s\": %.4f, \"upload_gbs\": %.3f}\n", total, read_s,
                    total / read_s / 1e9, up_s, total / up_s / 1e9);
        return 0;
    }
    const double t0 = now();
    CsvFileStream s(ctx, path, schema, batch, std::nullopt, CsvNulls::AsReference, mode == "device" ? CsvScan::Device : CsvScan::Host);
    size_t rows = 0, batches = 0;
    while (auto b = s.next_batch()) {
        rows += b->num_rows();
        ++batches;
    }
    check(rv_ctx_synchronize(ctx->raw()));
    const double secs = now() - t0;
    std::printf("{\"rows\": %zu, \"batches\": %zu, \"seconds\": %.4f, \"batch_rows\": %zu}\n", rows, batches, secs, s.batch_size());
    return 0;
}
