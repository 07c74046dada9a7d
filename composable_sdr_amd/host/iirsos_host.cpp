// iirsos_host kind design nchan chunks in out: the IirCFilter / IirFilterSOS pipes of csdr_host.hpp on a raw channel-major file
// ([nchan][n] of CF32 for kinds p and c, of F32 for kind r).  design is `n:fc` for p (the order-n Butterworth prototype) and
// `sos.f32` for r and c: a raw F32 file of S rows b0 b1 b2 a0 a1 a2 (scipy's sos layout).  chunks is a comma-separated list of call
// sizes in samples per row, used in turn and again from its start; the largest is the handle's max_samples.  Writes the rows of
// every call, row after row (tests/test_iirsos_gpu.py compares the bytes with the Python pipe's)
#include "host_driver.hpp"

using namespace csdrhost;

int main(int argc, char **argv)
{
    return driver_main("iirsos_host", "p|r|c n:fc|sos.f32 nchan chunks in out", argc, argv, 7, [&]() {
        const std::string kind = argv[1];
        const uint32_t nchan = std::atoi(argv[3]);
        const Chunks chunks(argv[4], nchan);
        const uint32_t max_in = chunks.largest();
        if (kind == "p") {
            const std::vector<std::string> d = split(argv[2], ':');
            if (d.size() != 2) throw std::runtime_error("bad design");
            run_rows(IirCFilter(std::atoi(d[0].c_str()), (float)std::atof(d[1].c_str()), 0.f, 10.f, 10.f, nchan, max_in), nchan, chunks, argv[5],
                     argv[6]);
        } else if (kind == "r" || kind == "c") {
            const Array<float> sos = read_all<float>(argv[2]);
            if (sos.empty() || sos.size() % 6) throw std::runtime_error("bad sos file");
            Array<float> b, a;
            for (size_t s = 0; s < sos.size() / 6; s++) {
                b.insert(b.end(), sos.begin() + 6 * s, sos.begin() + 6 * s + 3);
                a.insert(a.end(), sos.begin() + 6 * s + 3, sos.begin() + 6 * s + 6);
            }
            if (kind == "r") run_rows(IirFilterSOS<float>(b, a, nchan, max_in), nchan, chunks, argv[5], argv[6]);
            else run_rows(IirFilterSOS<cf32>(b, a, nchan, max_in), nchan, chunks, argv[5], argv[6]);
        } else throw std::runtime_error("bad kind");
    });
}
