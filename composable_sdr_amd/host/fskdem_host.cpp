// fskdem_host m k bw nchan chunk in.cf32 out.u32: the FskDemodulator pipe of csdr_host.hpp on a raw channel-major CF32 file
// ([nchan][n]), fed in calls of `chunk` samples per row; writes the symbols of every call, row after row, as raw uint32
// (tests/test_fskdem_gpu.py compares the bytes with the Python pipe's)
#include "host_driver.hpp"

using namespace csdrhost;

int main(int argc, char **argv)
{
    return driver_main("fskdem_host", "m k bw nchan chunk in.cf32 out.u32", argc, argv, 8, [&]() {
        const uint32_t m = std::atoi(argv[1]), k = std::atoi(argv[2]), nchan = std::atoi(argv[4]);
        const Chunks chunks(argv[5], nchan);
        run_rows(FskDemodulator(m, k, (float)std::atof(argv[3]), nchan, chunks.largest()), nchan, chunks, argv[6], argv[7]);
    });
}
