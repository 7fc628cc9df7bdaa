// The device PNG decoder's host-compilable code as a stand-alone program: the chunk walk behind bbocr_host_png_plan (csrc/png_parse.h) and
// the inflate the device runs (csrc/png_inflate.h: bit reader, table builder, symbol step) under its serial host driver.  Built with
// -fsanitize=address,undefined by tools/pngdec_hostcheck.py and run over the test files, damaged ones included: per file one line
//     <path> reason R status S produced P
// and, for a file the plan supports, <path>.raw = the P bytes the driver wrote.  No GPU, no HIP.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../bb-ocr_amd/csrc/png_inflate.h"
#include "../bb-ocr_amd/csrc/png_parse.h"

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
        png_host::PngParsed ps;
        const int reason = png_host::png_parse(file, data.size(), ps);
        int status = 0;
        size_t produced = 0;
        if (reason == BBOCR_PNG_OK) {
            const bbocr_png_plan& pl = ps.plan;
            const size_t expect = (size_t)pl.height * (size_t)(pl.row_bytes + 1);
            uint8_t* z = (uint8_t*)std::malloc((size_t)pl.idat_bytes);
            uint8_t* out = (uint8_t*)std::malloc(expect);
            png_host::png_gather(file, ps, z);
            status = pngi_inflate_zlib(z, (size_t)pl.idat_bytes, out, expect, &produced);
            FILE* o = std::fopen((std::string(argv[a]) + ".raw").c_str(), "wb");
            if (!o) return 2;
            std::fwrite(out, 1, produced, o);
            std::fclose(o);
            std::free(z);
            std::free(out);
        }
        std::free(file);
        std::printf("%s reason %d status %d produced %zu\n", argv[a], reason, status, produced);
    }
    return 0;
}
