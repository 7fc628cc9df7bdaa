// The device GIF decoder's host-compilable code as a stand-alone program: the walk behind bbocr_host_gif_plan (csrc/gif_parse.h) and what
// the kernels run -- the piece scan, the lengths pass, the offsets and the decode of every piece (csrc/gif_lzw.h) -- under their serial host
// drivers.  Built with -fsanitize=address,undefined by tools/gifdec_hostcheck.py and run over the test files, damaged and refused ones
// included: per file one line
//     <path> reason R status S pieces P total T
// and, for a file the plan supports, <path>.raw = the index stream (zero where nothing was decoded) and <path>.pieces = the piece table,
// 16 bytes per piece.  A path that ends in .bmp goes through the walk behind bbocr_host_bmp_plan (csrc/bmp_parse.h) instead, and every
// byte the BMP kernel would read -- the table, the rows -- is read here from an exact-size copy of the file (total = their sum modulo
// 2^32).  No GPU, no HIP.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../bb-ocr_amd/csrc/bmp_parse.h"
#include "../bb-ocr_amd/csrc/gif_lzw.h"
#include "../bb-ocr_amd/csrc/gif_parse.h"

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
        const std::string path = argv[a];
        if (path.size() > 4 && path.compare(path.size() - 4, 4, ".bmp") == 0) {
            bbocr_bmp_plan pl;
            const int reason = bmp_host::bmp_parse(file, data.size(), pl);
            uint32_t sum = 0;
            if (reason == BBOCR_BMP_OK) {
                for (long long i = 0; i < (long long)pl.table_entry * pl.colors; ++i) sum += file[pl.table_offset + i];
                for (long long i = 0; i < pl.row_stride * pl.height; ++i) sum += file[pl.data_offset + i];
            }
            std::free(file);
            std::printf("%s reason %d status 0 pieces 0 total %u\n", argv[a], reason, sum);
            continue;
        }
        gif_host::GifParsed ps;
        const int reason = gif_host::gif_parse(file, data.size(), ps);
        int status = 0;
        uint32_t count = 0, total = 0;
        if (reason == BBOCR_GIF_OK) {
            const bbocr_gif_plan& pl = ps.plan;
            const size_t bytes = ps.payload.size();
            const uint32_t need = (uint32_t)pl.width * (uint32_t)pl.height;
            const size_t cap = gifl_piece_room(bytes, pl.min_code);
            // exact-size copies of the payload, the tables and the stream, for the same reason
            uint8_t* in = (uint8_t*)std::malloc(bytes ? bytes : 1);
            if (bytes) std::memcpy(in, ps.payload.data(), bytes);
            GiflPiece* pieces = (GiflPiece*)std::malloc(sizeof(GiflPiece) * cap);
            uint32_t* lengths = (uint32_t*)std::calloc(cap, 4);
            int* errors = (int*)std::calloc(cap, 4);
            uint32_t* offsets = (uint32_t*)std::calloc(cap + 1, 4);
            uint8_t* stream = (uint8_t*)std::calloc(need, 1);
            const int scan_error = gifl_scan_host(in, bytes, pl.min_code, pieces, (uint32_t)cap, &count);
            for (uint32_t p = 0; p < count; ++p) errors[p] = gifl_lengths_host(in, bytes, pl.min_code, pieces[p], need, &lengths[p]);
            status = gifl_offsets_host(pieces, lengths, errors, count, scan_error, need, offsets);
            total = offsets[count];
            for (uint32_t p = 0; p < count && !scan_error; ++p) {        // (a damaged file's sound pieces too: the kernels skip such a file)
                if (offsets[p] >= need) break;
                uint32_t produced = 0;
                gifl_decode_host(in, bytes, pl.min_code, pieces[p], stream + offsets[p], need - offsets[p], &produced);
                if (produced != (lengths[p] < need - offsets[p] ? lengths[p] : need - offsets[p])) status |= 1 << 30;     // the two walks disagree
            }
            FILE* o = std::fopen((std::string(argv[a]) + ".raw").c_str(), "wb");
            if (!o) return 2;
            std::fwrite(stream, 1, need, o);
            std::fclose(o);
            o = std::fopen((std::string(argv[a]) + ".pieces").c_str(), "wb");
            if (!o) return 2;
            std::fwrite(pieces, sizeof(GiflPiece), count, o);
            std::fclose(o);
            std::free(in);
            std::free(pieces);
            std::free(lengths);
            std::free(errors);
            std::free(offsets);
            std::free(stream);
        }
        std::free(file);
        std::printf("%s reason %d status %d pieces %u total %u\n", argv[a], reason, status, count, total);
    }
    return 0;
}
