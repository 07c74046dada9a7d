// pfbsyn2_host M:m:as chunks in out: Firpfbch2Synthesizer behind Firpfbch2Channelizer (csdr_host.hpp) on a raw CF32 file, both
// with their own cutoff rule (fc = 0).  chunks is a comma-separated list of call sizes in frames (M / 2 samples each), used in
// turn and again from its start; the largest is the handles' max_frames; samples behind the last whole frame are dropped.
// Writes the re-assembled stream, as long as the input's whole frames and 2 M m - M / 2 + 1 samples late, to out as raw CF32
// (tests/test_pfbsyn2_gpu.py compares the bytes with the Python pipes')
#include "host_driver.hpp"

using namespace csdrhost;

int main(int argc, char **argv)
{
    return driver_main("pfbsyn2_host", "M:m:as chunks in out", argc, argv, 5, [&]() {
        const std::vector<std::string> d = split(argv[1], ':');
        if (d.size() != 3) throw std::runtime_error("bad design");
        const uint32_t M = std::atoi(d[0].c_str()), m = std::atoi(d[1].c_str());
        if (M < 2) throw std::runtime_error("bad M");
        const float as_db = (float)std::atof(d[2].c_str());
        const Chunks chunks(argv[2], 1);
        const Array<cf32> x = read_all<cf32>(argv[3]);
        const size_t P = M / 2, frames = x.size() / P;
        auto u = unPipe(compose(Firpfbch2Synthesizer(M, m, as_db, 0.f, chunks.largest()), Firpfbch2Channelizer(M, m, as_db, 0.f, chunks.largest())));
        std::FILE *o = std::fopen(argv[4], "wb");
        if (!o) throw std::runtime_error("cannot open output");
        size_t call = 0;
        for (size_t pos = 0; pos < frames; call++) {
            const size_t len = std::min(chunks.sizes[call % chunks.sizes.size()], frames - pos);
            const Array<cf32> y = u.process(Array<cf32>(x.begin() + pos * P, x.begin() + (pos + len) * P));
            std::fwrite(y.data(), sizeof(cf32), y.size(), o);
            pos += len;
        }
        u.cleanup();
        std::fclose(o);
    });
}
