// psktrack_host bits:sps:phase:eq_len:eq_mode nchan chunks in.cf32 out.cf32: the PskTracker pipe of csdr_host.hpp on a raw
// channel-major CF32 file ([nchan][n]), fed in calls of `chunks` samples per row; writes the soft symbols of every call, row after
// row, as raw CF32 (tests/test_psktrack_gpu.py compares the bytes with the Python pipe's).  m:k in place of the five numbers
// runs symTracker m k
#include "host_driver.hpp"

using namespace csdrhost;

int main(int argc, char **argv)
{
    return driver_main("psktrack_host", "bits:sps:phase:eq_len:eq_mode|m:k nchan chunks in.cf32 out.cf32", argc, argv, 6, [&]() {
        std::vector<uint32_t> p;
        for (const auto &v : split(argv[1], ':')) p.push_back((uint32_t)std::atoi(v.c_str()));
        if (p.size() != 5 && p.size() != 2) throw std::runtime_error("bad block arguments");
        const uint32_t nchan = std::atoi(argv[2]);
        const Chunks chunks(argv[3], nchan);
        run_rows(p.size() == 2 ? symTracker(p[0], p[1], nchan, chunks.largest()) : PskTracker(p[0], p[1], p[2], p[3], p[4], nchan, chunks.largest()),
                 nchan, chunks, argv[4], argv[5]);
    });
}
