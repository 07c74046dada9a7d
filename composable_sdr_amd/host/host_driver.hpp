// What the *_host test drivers share: each runs one row Pipe of csdr_host.hpp on a raw channel-major file ([nchan][n]), fed in
// calls of `chunks` samples per row, and writes the rows of every call, row after row; the tests compare the bytes with the
// Python pipe's.  A driver is its argument parsing and its choice of pipe.
#pragma once
#include <cstdlib>
#include <sstream>

#include "csdr_host.hpp"

namespace csdrhost {

inline std::vector<std::string> split(const std::string &s, char sep)
{
    std::vector<std::string> out;
    std::stringstream ss(s);
    for (std::string item; std::getline(ss, item, sep);) out.push_back(item);
    return out;
}

template <class T> Array<T> read_all(const char *path)
{
    std::FILE *f = std::fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    std::fseek(f, 0, SEEK_END);
    const size_t total = (size_t)std::ftell(f) / sizeof(T);
    std::fseek(f, 0, SEEK_SET);
    Array<T> x(total);
    const size_t got = std::fread(x.data(), sizeof(T), total, f);
    std::fclose(f);
    if (got != total) throw std::runtime_error("short read");
    return x;
}

// a comma-separated list of call sizes in samples per row (one number is a list of one), used in turn and again from its start;
// the largest is the handle's max_samples
struct Chunks {
    std::vector<size_t> sizes;
    Chunks(const char *list, uint32_t nchan)
    {
        for (const auto &c : split(list, ',')) sizes.push_back((size_t)std::atol(c.c_str()));
        if (sizes.empty() || !nchan || *std::min_element(sizes.begin(), sizes.end()) == 0) throw std::runtime_error("bad nchan or chunks");
    }
    uint32_t largest() const { return (uint32_t)*std::max_element(sizes.begin(), sizes.end()); }
};

template <class In, class Out> void run_rows(Pipe<Rows<In>, Rows<Out>> pipe, uint32_t nchan, const Chunks &chunks, const char *in, const char *out)
{
    const Array<In> x = read_all<In>(in);
    const size_t n = x.size() / nchan;
    auto u = unPipe(pipe);
    std::FILE *o = std::fopen(out, "wb");
    if (!o) throw std::runtime_error("cannot open output");
    size_t k = 0;
    for (size_t pos = 0; pos < n; k++) {
        const size_t len = std::min(chunks.sizes[k % chunks.sizes.size()], n - pos);
        Rows<In> rows;
        for (uint32_t c = 0; c < nchan; c++) rows.emplace_back(x.begin() + c * n + pos, x.begin() + c * n + pos + len);
        for (const auto &y : u.process(rows)) std::fwrite(y.data(), sizeof(Out), y.size(), o);
        pos += len;
    }
    u.cleanup();
    std::fclose(o);
}

// main's frame: `usage` and 2 for a wrong argument count, the exception's text and 1 for a failure
template <class Body> int driver_main(const char *name, const char *usage, int argc, char **argv, int want, Body body)
{
    if (argc != want) { std::fprintf(stderr, "usage: %s %s\n", argv[0], usage); return 2; }
    try {
        body();
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s: %s\n", name, e.what());
        return 1;
    }
    return 0;
}

}  // namespace csdrhost
