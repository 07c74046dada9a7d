// symsyncc_host m k nchan chunk in.cf32 out.cf32: the symSyncC pipe of csdr_host.hpp on a raw channel-major CF32 file
// ([nchan][n]), fed in calls of `chunk` samples per row; writes the symbols of every call, row after row, as raw CF32
// (tests/test_symsyncc_gpu.py compares the bytes with the Python pipe's)
#include "host_driver.hpp"

using namespace csdrhost;

int main(int argc, char **argv)
{
    return driver_main("symsyncc_host", "m k nchan chunk in.cf32 out.cf32", argc, argv, 7, [&]() {
        const uint32_t m = std::atoi(argv[1]), k = std::atoi(argv[2]), nchan = std::atoi(argv[3]);
        const Chunks chunks(argv[4], nchan);
        run_rows(symSyncC(m, k, nchan, chunks.largest()), nchan, chunks, argv[5], argv[6]);
    });
}
