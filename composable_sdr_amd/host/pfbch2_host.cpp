// pfbch2_host M:m:as:fc chunks in out: the Firpfbch2Channelizer pipe of csdr_host.hpp on a raw CF32 file.  chunks is a
// comma-separated list of call sizes in frames (M / 2 input samples each), used in turn and again from its start; the largest is
// the handle's max_frames; samples behind the last whole frame are dropped.  Writes <out>_ch<k>.cf32, k < M: row k of every call,
// call after call (tests/test_pfbch2_gpu.py compares the bytes with the Python pipe's)
#include "host_driver.hpp"

using namespace csdrhost;

int main(int argc, char **argv)
{
    return driver_main("pfbch2_host", "M:m:as:fc chunks in out", argc, argv, 5, [&]() {
        const std::vector<std::string> d = split(argv[1], ':');
        if (d.size() != 4) throw std::runtime_error("bad design");
        const uint32_t M = std::atoi(d[0].c_str()), m = std::atoi(d[1].c_str());
        if (M < 2) throw std::runtime_error("bad M");
        const Chunks chunks(argv[2], 1);
        const Array<cf32> x = read_all<cf32>(argv[3]);
        const size_t P = M / 2, frames = x.size() / P;
        auto u = unPipe(Firpfbch2Channelizer(M, m, (float)std::atof(d[2].c_str()), (float)std::atof(d[3].c_str()), chunks.largest()));
        std::vector<std::FILE *> outs;
        for (uint32_t k = 0; k < M; k++) {
            outs.push_back(std::fopen((std::string(argv[4]) + "_ch" + std::to_string(k) + ".cf32").c_str(), "wb"));
            if (!outs.back()) throw std::runtime_error("cannot open output");
        }
        size_t call = 0;
        for (size_t pos = 0; pos < frames; call++) {
            const size_t len = std::min(chunks.sizes[call % chunks.sizes.size()], frames - pos);
            const auto rows = u.process(Array<cf32>(x.begin() + pos * P, x.begin() + (pos + len) * P));
            for (uint32_t k = 0; k < M; k++) std::fwrite(rows[k].data(), sizeof(cf32), rows[k].size(), outs[k]);
            pos += len;
        }
        u.cleanup();
        for (std::FILE *f : outs) std::fclose(f);
    });
}
