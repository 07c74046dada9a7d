// rowresamp_host kind design nchan chunks in out: the RowResampler pipe of csdr_host.hpp on a raw channel-major file ([nchan][n] of
// F32 for kind r, of CF32 for kind c).  design is `rate:m:as:fc`.  chunks is a comma-separated list of call sizes in samples per
// row, used in turn and again from its start; the largest is the handle's max_samples.  Writes the rows of every call, row after
// row (tests/test_rowresamp_gpu.py compares the bytes with the Python pipe's)
#include "host_driver.hpp"

using namespace csdrhost;

int main(int argc, char **argv)
{
    return driver_main("rowresamp_host", "r|c rate:m:as:fc nchan chunks in out", argc, argv, 7, [&]() {
        const std::string kind = argv[1];
        const std::vector<std::string> d = split(argv[2], ':');
        if (d.size() != 4 || (kind != "r" && kind != "c")) throw std::runtime_error("bad kind or design");
        const double rate = std::atof(d[0].c_str());
        const uint32_t m = std::atoi(d[1].c_str()), nchan = std::atoi(argv[3]);
        const float as_db = (float)std::atof(d[2].c_str()), fc = (float)std::atof(d[3].c_str());
        const Chunks chunks(argv[4], nchan);
        if (kind == "c") run_rows(RowResampler<cf32>(rate, m, as_db, fc, nchan, chunks.largest()), nchan, chunks, argv[5], argv[6]);
        else run_rows(RowResampler<float>(rate, m, as_db, fc, nchan, chunks.largest()), nchan, chunks, argv[5], argv[6]);
    });
}
