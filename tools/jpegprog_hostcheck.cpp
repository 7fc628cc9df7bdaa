// The progressive scan decoder of csrc/jpegprog.h and the host side of csrc/jpeg_parse.h as a stand-alone host program, for a build with
// -fsanitize=address,undefined (tools/jpegprog_hostcheck.py builds and drives it): it plans every file named on the command line, decodes
// the scans of those the plan supports segment by segment -- the routine the device runs, one call where the device has one lane -- and
// writes the coefficients next to the file as FILE.coef (int16 [blocks][64]).  A first scan goes through jpeg_spec.h's subsequence lookup
// and packed state over cut_scan's tables; the baseline walk runs over every file as well (the walks share their pieces).  One line per
// file: its name, the baseline plan's reason, the progressive plan's reason, the decoder's JD_ERR_* bits.  Damaged files must end in a status, never in a report of the sanitisers.
#include <cstdio>
#include <string>
#include "../bb-ocr_amd/csrc/jpeg_parse.h"

using namespace jpeg_host;

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        std::vector<uint8_t> file;
        if (FILE* f = std::fopen(argv[a], "rb")) {
            uint8_t buf[65536];
            for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) file.insert(file.end(), buf, buf + n);
            std::fclose(f);
        }
        JpegParsed base;                                                  // the baseline walk over the same bytes: the shared pieces' other user
        const int base_reason = jpeg_parse(file.data(), file.size(), base, true);
        ProgParsed pp;
        const int reason = prog_parse(file.data(), file.size(), pp, true);
        if (reason != BBOCR_JPEG_OK) {
            std::printf("%s baseline %d reason %d\n", argv[a], base_reason, reason);
            continue;
        }
        const bbocr_jpeg_progressive_plan& pl = pp.plan;
        std::vector<short> coef;
        int status = 0;
        for (int k = 0; k < pl.n_scans; ++k) {
            const int S = 1024;
            std::vector<uint8_t> data((size_t)pl.scans[k].bytes + 8);
            std::vector<int> seg_byte((size_t)pl.scans[k].segments + 1), seg_sub((size_t)pl.scans[k].segments + 1);
            std::vector<int> sub_seg(prog_scan_subs(pl.scans[k], S) + 1);
            JpegHuff huff[3];
            JpScan sc{};
            prog_fill_scan(pp, k, file.data(), S, data.data(), seg_byte.data(), huff, seg_sub.data(), sub_seg.data(), sc);
            if (coef.empty()) coef.assign((size_t)sc.nblocks * 64, 0);
            sc.data = data.data();
            sc.seg_byte = seg_byte.data();
            sc.seg_sub = seg_sub.data();
            sc.sub_seg = sub_seg.data();
            sc.huff = huff;
            sc.coef = coef.data();
            sc.status = &status;
            for (int g = 0; g < sc.nseg; ++g) status |= jp_decode_segment(sc, huff, JPEG_ZZ, g);
        }
        if (FILE* f = std::fopen((std::string(argv[a]) + ".coef").c_str(), "wb")) {
            std::fwrite(coef.data(), 2, coef.size(), f);
            std::fclose(f);
        }
        std::printf("%s baseline %d reason 0 status %d\n", argv[a], base_reason, status);
    }
    return 0;
}
