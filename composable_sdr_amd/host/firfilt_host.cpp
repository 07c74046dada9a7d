// firfilt_host kind design nchan chunks in out: the FirFilterR / FirFilterC / FirFilterCKaiser pipes of csdr_host.hpp on a raw
// channel-major file ([nchan][n] of F32 for kind r, of CF32 for kinds c and k).  design is `taps.f32:scale` (a raw F32 file of
// taps and the scale) for r and c, and `n:fc:as` for k.  chunks is a comma-separated list of call sizes in samples per row, used
// in turn and again from its start; the largest is the handle's max_samples.  Writes the rows of every call, row after row
// (tests/test_firfilt_gpu.py compares the bytes with the Python pipe's)
#include "host_driver.hpp"

using namespace csdrhost;

int main(int argc, char **argv)
{
    return driver_main("firfilt_host", "r|c|k taps.f32:scale|n:fc:as nchan chunks in out", argc, argv, 7, [&]() {
        const std::string kind = argv[1];
        const std::vector<std::string> d = split(argv[2], ':');
        const uint32_t nchan = std::atoi(argv[3]);
        const Chunks chunks(argv[4], nchan);
        const uint32_t max_in = chunks.largest();
        if (kind == "k" && d.size() == 3)
            run_rows(FirFilterCKaiser(std::atoi(d[0].c_str()), (float)std::atof(d[1].c_str()), (float)std::atof(d[2].c_str()), 0.f, nchan, max_in),
                     nchan, chunks, argv[5], argv[6]);
        else if ((kind == "r" || kind == "c") && d.size() == 2) {
            const Array<float> taps = read_all<float>(d[0].c_str());
            const float scale = (float)std::atof(d[1].c_str());
            if (kind == "r") run_rows(FirFilterR(taps, scale, nchan, max_in), nchan, chunks, argv[5], argv[6]);
            else run_rows(FirFilterC(taps, scale, nchan, max_in), nchan, chunks, argv[5], argv[6]);
        } else throw std::runtime_error("bad kind or design");
    });
}
