// symsyncc_host m k nchan chunk in.cf32 out.cf32: the symSyncC pipe of csdr_host.hpp on a raw channel-major CF32 file
// ([nchan][n]), fed in calls of `chunk` samples per row; writes the symbols of every call, row after row, as raw CF32
// (tests/test_symsyncc_gpu.py compares the bytes with the Python pipe's)
#include "csdr_host.hpp"

#include <algorithm>
#include <cstdlib>

using namespace csdrhost;

int main(int argc, char **argv)
{
    if (argc != 7) { std::fprintf(stderr, "usage: %s m k nchan chunk in.cf32 out.cf32\n", argv[0]); return 2; }
    const uint32_t m = std::atoi(argv[1]), k = std::atoi(argv[2]), nchan = std::atoi(argv[3]), chunk = std::atoi(argv[4]);
    try {
        std::FILE *f = std::fopen(argv[5], "rb");
        if (!f) throw std::runtime_error("cannot open input");
        std::fseek(f, 0, SEEK_END);
        const size_t total = (size_t)std::ftell(f) / sizeof(cf32), n = total / nchan;
        std::fseek(f, 0, SEEK_SET);
        Array<cf32> x(total);
        if (std::fread(x.data(), sizeof(cf32), total, f) != total) throw std::runtime_error("short read");
        std::fclose(f);
        auto u = unPipe(symSyncC(m, k, nchan, chunk));
        std::FILE *o = std::fopen(argv[6], "wb");
        if (!o) throw std::runtime_error("cannot open output");
        for (size_t pos = 0; pos < n; pos += chunk) {
            const size_t len = std::min<size_t>(chunk, n - pos);
            std::vector<Array<cf32>> rows;
            for (uint32_t c = 0; c < nchan; c++) rows.emplace_back(x.begin() + c * n + pos, x.begin() + c * n + pos + len);
            for (const auto &s : u.process(rows)) std::fwrite(s.data(), sizeof(cf32), s.size(), o);
        }
        u.cleanup();
        std::fclose(o);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "symsyncc_host: %s\n", e.what());
        return 1;
    }
    return 0;
}
