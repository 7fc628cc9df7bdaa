// The CCITT side of the device TIFF decoder as a stand-alone program: the lenient IFD walk and the fax checks behind
// bbocr_host_tiff_fax_plan (csrc/tiff_parse.h) and the strip decoder the device runs (csrc/tiff_fax.h) under its serial policy.  Built with
// -fsanitize=address,undefined by tools/tiff_fax_hostcheck.py and run over the files of tests/tiff_fax_ref.py, damaged and refused ones
// included: per file one line
//     <path> reason R fax F scheme S status T produced P
// and, for a CCITT file the plan supports, <path>.raw = the strips' decoded stream (a damaged strip's bytes are left zero).  No GPU, no HIP.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../bb-ocr_amd/csrc/tiff_fax.h"
#include "../bb-ocr_amd/csrc/tiff_parse.h"

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        FILE* f = std::fopen(argv[a], "rb");
        if (!f) return 2;
        std::vector<uint8_t> data;
        uint8_t buf[65536];
        for (size_t got; (got = std::fread(buf, 1, sizeof buf, f)) > 0;) data.insert(data.end(), buf, buf + got);
        std::fclose(f);
        // an exact-size heap copy: a read one byte past the file is a sanitizer report
        uint8_t* file = (uint8_t*)std::malloc(data.size() ? data.size() : 1);
        if (!data.empty()) std::memcpy(file, data.data(), data.size());
        tiff_host::TiffParsed ps;
        bbocr_tiff_fax fax;
        const bool takes = tiff_host::tiff_fax_parse(file, data.size(), ps, fax);
        int status = 0;
        size_t produced = 0;
        if (takes && fax.scheme) {
            const bbocr_tiff_plan& pl = ps.plan;
            const size_t total = (size_t)pl.height * (size_t)pl.row_bytes;
            std::vector<uint8_t> stream(total, 0);
            for (size_t s = 0; s < ps.strips.size(); ++s) {
                const long long rows = tiff_host::tiff_strip_rows(pl, (int)s);
                const size_t need = (size_t)rows * (size_t)pl.row_bytes, n = ps.strips[s].second;
                // exact-size copies of the strip and of its output, for the same reason
                uint8_t* in = (uint8_t*)std::malloc(n ? n : 1);
                uint8_t* out = (uint8_t*)std::calloc(need ? need : 1, 1);
                std::memcpy(in, file + ps.strips[s].first, n);
                const int err = fax_decode_strip_host(in, n, out, pl.width, (int)rows, fax.scheme, fax.t4_options, fax.fill_order);
                if (!err) {
                    std::memcpy(stream.data() + s * (size_t)pl.rows_per_strip * (size_t)pl.row_bytes, out, need);
                    produced += need;
                }
                status |= err;
                std::free(in);
                std::free(out);
            }
            FILE* o = std::fopen((std::string(argv[a]) + ".raw").c_str(), "wb");
            if (!o) return 2;
            std::fwrite(stream.data(), 1, total, o);
            std::fclose(o);
        }
        std::free(file);
        std::printf("%s reason %d fax %d scheme %d status %d produced %zu\n", argv[a], ps.plan.reason, fax.reason, fax.scheme, status, produced);
    }
    return 0;
}
