// iirsos_host kind design nchan chunks in out: the IirCFilter / IirFilterSOS pipes of csdr_host.hpp on a raw channel-major file
// ([nchan][n] of CF32 for kinds p and c, of F32 for kind r).  design is `n:fc` for p (the order-n Butterworth prototype) and
// `sos.f32` for r and c: a raw F32 file of S rows b0 b1 b2 a0 a1 a2 (scipy's sos layout).  chunks is a comma-separated list of call
// sizes in samples per row, used in turn and again from its start; the largest is the handle's max_samples.  Writes the rows of
// every call, row after row (tests/test_iirsos_gpu.py compares the bytes with the Python pipe's)
#include "csdr_host.hpp"

#include <algorithm>
#include <cstdlib>
#include <sstream>

using namespace csdrhost;

static std::vector<std::string> split(const std::string &s, char sep)
{
    std::vector<std::string> out;
    std::stringstream ss(s);
    for (std::string item; std::getline(ss, item, sep);) out.push_back(item);
    return out;
}

template <class T> static Array<T> read_all(const char *path)
{
    std::FILE *f = std::fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    std::fseek(f, 0, SEEK_END);
    const size_t total = (size_t)std::ftell(f) / sizeof(T);
    std::fseek(f, 0, SEEK_SET);
    Array<T> x(total);
    if (std::fread(x.data(), sizeof(T), total, f) != total) throw std::runtime_error("short read");
    std::fclose(f);
    return x;
}

template <class T> static void run(Pipe<std::vector<Array<T>>, std::vector<Array<T>>> pipe, uint32_t nchan, const std::vector<size_t> &chunks,
                                   const char *in, const char *out)
{
    const Array<T> x = read_all<T>(in);
    const size_t n = x.size() / nchan;
    auto u = unPipe(pipe);
    std::FILE *o = std::fopen(out, "wb");
    if (!o) throw std::runtime_error("cannot open output");
    size_t k = 0;
    for (size_t pos = 0; pos < n; k++) {
        const size_t len = std::min(chunks[k % chunks.size()], n - pos);
        std::vector<Array<T>> rows;
        for (uint32_t c = 0; c < nchan; c++) rows.emplace_back(x.begin() + c * n + pos, x.begin() + c * n + pos + len);
        for (const auto &y : u.process(rows)) std::fwrite(y.data(), sizeof(T), y.size(), o);
        pos += len;
    }
    u.cleanup();
    std::fclose(o);
}

int main(int argc, char **argv)
{
    if (argc != 7) { std::fprintf(stderr, "usage: %s p|r|c n:fc|sos.f32 nchan chunks in out\n", argv[0]); return 2; }
    try {
        const std::string kind = argv[1];
        const uint32_t nchan = std::atoi(argv[3]);
        std::vector<size_t> chunks;
        for (const auto &c : split(argv[4], ',')) chunks.push_back((size_t)std::atol(c.c_str()));
        if (chunks.empty() || !nchan || *std::min_element(chunks.begin(), chunks.end()) == 0) throw std::runtime_error("bad nchan or chunks");
        const uint32_t max_in = (uint32_t)*std::max_element(chunks.begin(), chunks.end());
        if (kind == "p") {
            const std::vector<std::string> d = split(argv[2], ':');
            if (d.size() != 2) throw std::runtime_error("bad design");
            run<cf32>(IirCFilter(std::atoi(d[0].c_str()), (float)std::atof(d[1].c_str()), 0.f, 10.f, 10.f, nchan, max_in), nchan, chunks, argv[5],
                      argv[6]);
        } else if (kind == "r" || kind == "c") {
            const Array<float> sos = read_all<float>(argv[2]);
            if (sos.empty() || sos.size() % 6) throw std::runtime_error("bad sos file");
            Array<float> b, a;
            for (size_t s = 0; s < sos.size() / 6; s++) {
                b.insert(b.end(), sos.begin() + 6 * s, sos.begin() + 6 * s + 3);
                a.insert(a.end(), sos.begin() + 6 * s + 3, sos.begin() + 6 * s + 6);
            }
            if (kind == "r") run<float>(IirFilterSOS<float>(b, a, nchan, max_in), nchan, chunks, argv[5], argv[6]);
            else run<cf32>(IirFilterSOS<cf32>(b, a, nchan, max_in), nchan, chunks, argv[5], argv[6]);
        } else throw std::runtime_error("bad kind");
    } catch (const std::exception &e) {
        std::fprintf(stderr, "iirsos_host: %s\n", e.what());
        return 1;
    }
    return 0;
}
