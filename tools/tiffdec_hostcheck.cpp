// The device TIFF decoder's host-compilable code as a stand-alone program: the IFD walk behind bbocr_host_tiff_plan (csrc/tiff_parse.h) and
// the strip decoders the device runs (csrc/tiff_codecs.h: PackBits, LZW; csrc/png_inflate.h: Deflate) under their serial host drivers.
// Built with -fsanitize=address,undefined by tools/tiffdec_hostcheck.py and run over the test files, damaged and refused ones included: per
// file one line
//     <path> reason R status S produced P
// and, for a file the plan supports, <path>.raw = the strips' decoded stream (a damaged strip's bytes are left zero).  No GPU, no HIP.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../bb-ocr_amd/csrc/png_inflate.h"
#include "../bb-ocr_amd/csrc/tiff_codecs.h"
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
        const int reason = tiff_host::tiff_parse(file, data.size(), ps);
        int status = 0;
        size_t produced = 0;
        if (reason == BBOCR_TIFF_OK) {
            const bbocr_tiff_plan& pl = ps.plan;
            const size_t total = (size_t)pl.height * (size_t)pl.row_bytes;
            std::vector<uint8_t> stream(total, 0);
            for (size_t s = 0; s < ps.strips.size(); ++s) {
                const size_t need = (size_t)tiff_host::tiff_strip_rows(pl, (int)s) * (size_t)pl.row_bytes;
                // exact-size copies of the strip and of its output, for the same reason
                uint8_t* in = (uint8_t*)std::malloc(ps.strips[s].second ? ps.strips[s].second : 1);
                uint8_t* out = (uint8_t*)std::calloc(need ? need : 1, 1);
                std::memcpy(in, file + ps.strips[s].first, ps.strips[s].second);
                const size_t n = ps.strips[s].second;
                int err = 0;
                if (pl.compression == 1) {
                    if (n < need) err = TIFFC_ERR_INPUT;
                    else std::memcpy(out, in, need);
                } else if (pl.compression == 32773) {
                    err = tiffc_packbits_host(in, n, out, need);
                } else if (pl.compression == 5) {
                    err = tiffc_lzw_host(in, n, out, need);
                } else {
                    size_t got = 0;
                    err = pngi_inflate_zlib(in, n, out, need, &got);
                }
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
        std::printf("%s reason %d status %d produced %zu\n", argv[a], reason, status, produced);
    }
    return 0;
}
