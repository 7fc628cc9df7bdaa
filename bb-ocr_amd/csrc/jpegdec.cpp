// Baseline JPEG decoding, host side: the marker parser (bbocr_host_jpeg_plan: one linear pass, no entropy bit decoded), the per-batch
// tables of jpegdec.hip (unstuffed segment bytes, subsequence lists, derived Huffman tables) and its launch sequence.  A batch runs on
// its own stream of the root context, outside the call slots (the contract of bbocr_upload_pages): files decode while two OCR calls run.
// A batch runs the entropy stages once per file and one IDCT + output pass per requested output: scale 1, or 1/2, 1/4, 1/8 (Pillow's
// draft); YCbCr pixels or, at scale 1, the oriented BGR page of cv2.imread.  jpeg_geometry is the one statement of what a scale and a
// sampling mean for a pass -- block edges, planes, valid extents, upsampling rule; the device reads it from the descriptors, the plane
// sizes and bbocr_host_jpeg_scaled_geometry are taken from it.  Every pixel entry point is jpeg_decode_outputs with its own list of
// outputs (bbocr_jpeg_decode_scaled refuses the files of a chroma class at a draft scale: its documented scope), every stage entry point
// jpeg_stage_run.  A progressive file (bbocr_jpeg_decode_progressive alone admits one) is a job whose frame is a plan without a scan -- the
// baseline entropy stages find nothing to do for it -- and whose scans (jpeg_parse.h) run through jpegprog.hip's launches instead, level
// by level, into the same coefficient buffer; everything behind the coefficients is shared.
#include "ctx.h"
#include "jpeg_parse.h"

namespace {

using namespace jpeg_host;

struct JpegParsed {
    bbocr_jpeg_plan plan{};
    unsigned short quant[3][64];              // per component, natural order
    HuffSpec huff[2][2];                      // [class][id]
    int tab_dc[3], tab_ac[3];
    std::vector<std::pair<size_t, size_t>> segs;   // byte ranges of the restart segments in the file (stuffing included)
};

// The chroma layouts outside `supported` that the decoder takes all the same (bbocr_jpeg_plan::chroma): luma (1,1), (2,1) or (1,2) over
// chroma (1,1), (1,1).  0: any other sampling.
int chroma_class(const bbocr_jpeg_plan& pl) { return chroma_class_of(pl.sampling); }

// jdmarker.c's walk over the headers up to SOS, then over the entropy-coded data up to the marker that ends it.  Returns the reason;
// `cls` receives the chroma class of a file whose sampling alone is outside today's scope, and the walk goes on as for a supported file.
int jpeg_walk(const uint8_t* f, size_t n, JpegParsed& out, bool want_segs, int& cls) {
    bbocr_jpeg_plan& pl = out.plan;
    pl = bbocr_jpeg_plan{};
    if (n < 4 || f[0] != 0xFF || f[1] != 0xD8) return BBOCR_JPEG_NOT_JPEG;
    pl.orientation = exif_orientation(f, n);                     // of its own walk: malformed EXIF never changes what follows
    size_t p = 2;
    unsigned short qt[4][64];
    bool have_qt[4] = {false, false, false, false};
    bool have_sof = false, jfif = false;
    int adobe = -1, comp_id[4] = {0}, comp_tq[4] = {0}, dri = 0;
    size_t scan_off = 0;
    for (;;) {
        for (;;) {
            if (p + 2 > n || f[p] != 0xFF) return BBOCR_JPEG_TRUNCATED;
            if (f[p + 1] == 0xFF) { ++p; continue; }
            break;
        }
        const int m = f[p + 1];
        p += 2;
        if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;
        if (m == 0xD9) return BBOCR_JPEG_TRUNCATED;
        if (p + 2 > n) return BBOCR_JPEG_TRUNCATED;
        const size_t L = ((size_t)f[p] << 8) | f[p + 1];
        if (L < 2 || p + L > n) return BBOCR_JPEG_TRUNCATED;
        const uint8_t* s = f + p + 2;
        const size_t sl = L - 2;
        if (m == 0xC0) {
            if (have_sof || sl < 6) return BBOCR_JPEG_SOF;
            if (s[0] != 8) return BBOCR_JPEG_PRECISION;
            pl.height = (s[1] << 8) | s[2];
            pl.width = (s[3] << 8) | s[4];
            pl.components = s[5];
            if (pl.height == 0 || pl.width == 0 || sl < 6 + 3 * (size_t)pl.components) return BBOCR_JPEG_SOF;
            for (int i = 0; i < pl.components && i < 4; ++i) {
                comp_id[i] = s[6 + 3 * i];
                if (i < 3) { pl.sampling[i][0] = s[7 + 3 * i] >> 4; pl.sampling[i][1] = s[7 + 3 * i] & 15; }
                comp_tq[i] = s[8 + 3 * i];
            }
            have_sof = true;
        } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8) {
            return BBOCR_JPEG_SOF;                           // extended, progressive, lossless, arithmetic conditioning
        } else if (m == 0xC4) {
            if (!read_dht(s, sl, out.huff)) return BBOCR_JPEG_TABLES;
        } else if (m == 0xDB) {
            size_t q = 0;
            while (q < sl) {
                if (s[q] >> 4) return BBOCR_JPEG_PRECISION;
                const int id = s[q] & 15;
                if (id > 3 || q + 65 > sl) return BBOCR_JPEG_TABLES;
                for (int k = 0; k < 64; ++k) qt[id][kZigzag[k]] = s[q + 1 + k];
                have_qt[id] = true;
                q += 65;
            }
        } else if (m == 0xDD) {
            if (sl < 2) return BBOCR_JPEG_TRUNCATED;
            dri = (s[0] << 8) | s[1];
        } else if (m == 0xE0 && sl >= 5 && std::memcmp(s, "JFIF\0", 5) == 0) {
            jfif = true;
        } else if (m == 0xEE && sl >= 12 && std::memcmp(s, "Adobe", 5) == 0) {
            adobe = s[11];
        } else if (m == 0xDA) {
            if (!have_sof) return BBOCR_JPEG_SOF;
            const int nc = pl.components;
            if (nc != 1 && nc != 3) return BBOCR_JPEG_COMPONENTS;
            if (nc == 3) {
                if (!jfif && adobe != 1) return BBOCR_JPEG_COLORSPACE;
                if (pl.sampling[0][0] != 2 || pl.sampling[0][1] != 2 || pl.sampling[1][0] != 1 || pl.sampling[1][1] != 1 || pl.sampling[2][0] != 1 ||
                    pl.sampling[2][1] != 1) {
                    cls = chroma_class(pl);
                    if (!cls) return BBOCR_JPEG_SAMPLING;
                }
            }
            if (sl < 1 || s[0] != nc || sl < 1 + 2 * (size_t)nc + 3) return BBOCR_JPEG_MULTISCAN;
            for (int i = 0; i < nc; ++i) {
                if (s[1 + 2 * i] != comp_id[i]) return BBOCR_JPEG_MULTISCAN;
                const int td = s[2 + 2 * i] >> 4, ta = s[2 + 2 * i] & 15;
                if (td > 1 || ta > 1 || !out.huff[0][td].have || !out.huff[1][ta].have || comp_tq[i] > 3 || !have_qt[comp_tq[i]]) return BBOCR_JPEG_TABLES;
                out.tab_dc[i] = td;
                out.tab_ac[i] = 2 + ta;
                std::memcpy(out.quant[i], qt[comp_tq[i]], sizeof qt[0]);
            }
            scan_off = p + L;
            break;
        }
        p += L;
    }
    const int mcu_w = pl.components == 3 ? 8 * pl.sampling[0][0] : 8, mcu_h = pl.components == 3 ? 8 * pl.sampling[0][1] : 8;
    pl.mcu_cols = (pl.width + mcu_w - 1) / mcu_w;
    pl.mcu_rows = (pl.height + mcu_h - 1) / mcu_h;
    pl.restart_interval = dri;
    pl.scan_offset = (long long)scan_off;
    const long long nmcu = (long long)pl.mcu_cols * pl.mcu_rows;
    size_t end = 0;
    int nseg = 0;
    const int walked = scan_segments(f, n, scan_off, want_segs, out.segs, nseg, end);
    if (walked != BBOCR_JPEG_OK) return walked;
    if (f[end + 1] != 0xD9) return BBOCR_JPEG_MULTISCAN;
    const long long ri = dri ? dri : nmcu;
    if ((long long)nseg != (nmcu + ri - 1) / ri) return BBOCR_JPEG_RESTART;
    pl.segments = nseg;
    pl.scan_bytes = (long long)(end - scan_off);
    return BBOCR_JPEG_OK;
}

// The plan of a file and its reason.  A file of a chroma class that passed every later check keeps reason BBOCR_JPEG_SAMPLING and
// supported 0, with `chroma` set and the whole plan filled; one that failed a later check is refused as before, nothing behind the
// sampling test filled.
int jpeg_parse(const uint8_t* f, size_t n, JpegParsed& out, bool want_segs) {
    int cls = 0;
    const int reason = jpeg_walk(f, n, out, want_segs, cls);
    bbocr_jpeg_plan& pl = out.plan;
    pl.supported = reason == BBOCR_JPEG_OK && !cls;
    if (!cls) return reason;
    if (reason == BBOCR_JPEG_OK) {
        pl.chroma = cls;
    } else {
        pl.restart_interval = pl.mcu_cols = pl.mcu_rows = pl.segments = 0;
        pl.scan_offset = pl.scan_bytes = 0;
    }
    return BBOCR_JPEG_SAMPLING;
}

// the decoder takes the file: inside today's scope, or of a chroma class
bool jpeg_taken(const bbocr_jpeg_plan& pl) { return pl.supported || pl.chroma; }

// luma blocks of an MCU across and down (1 x 1 for a one-component file)
int luma_h(const bbocr_jpeg_plan& pl) { return pl.components == 3 ? pl.sampling[0][0] : 1; }
int luma_v(const bbocr_jpeg_plan& pl) { return pl.components == 3 ? pl.sampling[0][1] : 1; }
bool jpeg_scale_ok(int s) { return s == 1 || s == 2 || s == 4 || s == 8; }
int scaled_dim(int v, int s) { return (v + s - 1) / s; }

static_assert((int)JD_UP_NONE == (int)BBOCR_JPEG_UP_NONE && (int)JD_UP_H2V1_FANCY == (int)BBOCR_JPEG_UP_H2V1_FANCY &&
                  (int)JD_UP_H1V2_FANCY == (int)BBOCR_JPEG_UP_H1V2_FANCY && (int)JD_UP_H2V2_NOT_NEEDED == (int)BBOCR_JPEG_UP_H2V2_NOT_NEEDED &&
                  (int)JD_UP_REPLICATE == (int)BBOCR_JPEG_UP_REPLICATE,
              "kernels.h's JD_UP_* begin with bbocr.h's BBOCR_JPEG_UP_*");

// A decode at scale 1 / s (s 1, 2, 4 or 8) of a file the decoder takes: OH x OW pixels and, per component, the geometry of jpegdec.hip's
// IDCT + output pass.  jdmaster.c gives a component the block edge n = 8 / s, and twice that when its sampling is below luma's in BOTH
// directions and n < 8 -- 4:2:0 chroma at a draft scale, whose plane then has the output's size.  Everywhere else chroma keeps the file's
// sampling: planes of whole MCUs of one n x n block, the valid extent ceil(OH / v) x ceil(OW / h), brought to the output's size by
// jdsample.c's fancy upsampling (by replication at s = 8: min_DCT_scaled_size 1 turns the fancy kind off).
struct JpegGeometry { int OH, OW; JpegComp comp[3]; };
JpegGeometry jpeg_geometry(const bbocr_jpeg_plan& pl, int s) {
    JpegGeometry g{};
    const int n = 8 / s, h = luma_h(pl), v = luma_v(pl), oh = g.OH = scaled_dim(pl.height, s), ow = g.OW = scaled_dim(pl.width, s);
    g.comp[0] = {n, h, v, pl.mcu_rows * n * v, pl.mcu_cols * n * h, oh, ow, JD_UP_NONE};
    for (int c = 1; c < pl.components; ++c) {
        if (h * v == 4 && s > 1) {
            g.comp[c] = {2 * n, 1, 1, pl.mcu_rows * 2 * n, pl.mcu_cols * 2 * n, oh, ow, JD_UP_H2V2_NOT_NEEDED};
            continue;
        }
        const int up = h * v == 1 ? JD_UP_NONE : (s == 8 ? JD_UP_REPLICATE : (h * v == 4 ? JD_UP_H2V2_FANCY : (h == 2 ? JD_UP_H2V1_FANCY : JD_UP_H1V2_FANCY)));
        g.comp[c] = {n, 1, 1, pl.mcu_rows * n, pl.mcu_cols * n, scaled_dim(oh, v), scaled_dim(ow, h), up};
    }
    return g;
}
size_t plane_size(const JpegComp& c) { return (size_t)c.plane_rows * (size_t)c.pitch; }

constexpr int kMaxPasses = 4;                 // IDCT + output passes over one batch's coefficients: one per scale
struct JpegPass { int scale, px; };           // px: bytes per pixel of a 3-component file's output

struct FileJob {                              // one admitted file of a batch
    JpegParsed ps;
    const uint8_t* file = nullptr;            // its bytes (caller-owned)
    uint8_t* out[kMaxPasses] = {nullptr};     // per pass: where the decoder writes its pixels, rows `pitch` bytes apart
    long long pitch[kMaxPasses] = {0};
    int k = 0;                                // its index in the caller's arrays (status[])
    int nsub = 0, groups = 0, nblocks = 0;
    size_t o_huff, o_quant, o_segbyte, o_segsub, o_subseg, o_data, data_bytes;   // offsets in the input blob
    size_t w_entry, w_exits, w_count, w_scan, w_first, w_flags, w_plane[kMaxPasses][3], o_coef; // offsets in the work / coefficient buffers
    size_t o_page = 0;                        // the imread form: offset of the un-oriented decode in jd_page
    JpegGeometry geo[kMaxPasses];             // per pass (filled by jpeg_run)
    std::shared_ptr<ProgParsed> prog;         // a progressive file: its scans; `ps` then holds the frame alone, as a plan without a scan
    struct ScanBlob { size_t o_data, o_segbyte, o_huff, o_segsub, o_subseg, subs, w_entry, w_exits, w_count, w_scan, w_flags; };
    std::vector<ScanBlob> scan_blob;          // per scan: offsets in the input blob
};

// The frame of a progressive file the plan supports as the stages behind the entropy side read it: a baseline plan of the same size and
// sampling without a scan (0 segments, 0 bytes), so that the baseline entropy stages find nothing to do for it.
void frame_of(const ProgParsed& pp, JpegParsed& ps) {
    const bbocr_jpeg_progressive_plan& q = pp.plan;
    bbocr_jpeg_plan& pl = ps.plan;
    pl = bbocr_jpeg_plan{};
    pl.width = q.width;
    pl.height = q.height;
    pl.components = q.components;
    std::memcpy(pl.sampling, q.sampling, sizeof pl.sampling);
    pl.mcu_cols = q.mcu_cols;
    pl.mcu_rows = q.mcu_rows;
    pl.orientation = q.orientation;
    pl.chroma = q.chroma;
    pl.supported = !q.chroma;
    std::memcpy(ps.quant, pp.quant, sizeof ps.quant);
    for (int c = 0; c < 3; ++c) ps.tab_dc[c] = ps.tab_ac[c] = 0;
    ps.segs.clear();
}

// Admission of a batch: status[k] = BBOCR_ERR_ARG for a null or oversized file and for one the plan neither supports nor gives a chroma
// class (the caller plans first: a refused file is its error); every other file becomes a job once dest(job) -- the entry point's own rule -- has checked the caller's
// destination and set the job's `out` and `pitch` (false: refused like the others).  chroma_classes false (a scaled decode): only the
// files the plan supports, 4:2:0 and grey.  progressive: a file both refuse is planned as a progressive one
// (bbocr_host_jpeg_progressive_plan) and admitted when that plan supports it.
template <typename D> std::vector<FileJob> jpeg_admit(const uint8_t* const* files, const size_t* bytes, int n, int* status, D&& dest,
                                                       bool chroma_classes = true, bool progressive = false) {
    std::vector<FileJob> jobs;
    jobs.reserve((size_t)n);
    for (int k = 0; k < n; ++k) {
        status[k] = BBOCR_ERR_ARG;
        if (!files[k] || bytes[k] >= ((size_t)1 << 28)) continue;
        FileJob j;
        const int reason = jpeg_parse(files[k], bytes[k], j.ps, true);
        if (progressive && !jpeg_taken(j.ps.plan) && reason != BBOCR_JPEG_NOT_JPEG) {   // whatever the baseline walk stopped at
            j.prog = std::make_shared<ProgParsed>();
            if (prog_parse(files[k], bytes[k], *j.prog, true) != BBOCR_JPEG_OK) continue;
            frame_of(*j.prog, j.ps);
        }
        if (!jpeg_taken(j.ps.plan) || (!chroma_classes && !j.ps.plan.supported)) continue;
        j.file = files[k];
        j.k = k;
        if (dest(j)) jobs.push_back(std::move(j));
    }
    return jobs;
}

// the decoder's verdict on each job (jpeg_run's dev_status) as the caller's status
void jpeg_report(const std::vector<FileJob>& jobs, const std::vector<int>& dev_status, int* status) {
    for (size_t i = 0; i < jobs.size(); ++i) status[jobs[i].k] = dev_status[i] ? BBOCR_ERR_DATA : BBOCR_OK;
}

// The whole decode of the admitted jobs on the JPEG lane's stream `st`.  Fills dev_status[i] (JD_ERR_* bits of job i) and leaves the
// descriptors of the first pass for the stage entry points.  Everything queued is finished on return.
// The entropy stages run once; then every pass (at most kMaxPasses) runs its IDCT and output stage over the shared coefficients into
// planes of its own and the jobs' out[p] / pitch[p].  A pass of scale 2, 4 or 8 is the decode at that fraction (`out[p]` holds the scaled
// size); its descriptors carry jpeg_geometry's table, so one launch pair serves every file of the batch.
void jpeg_run(bbocr_ctx* root, hipStream_t st, std::vector<FileJob>& jobs, int S, const std::vector<JpegPass>& passes_out,
              std::vector<int>& dev_status, std::vector<JpegDesc>* descs_out = nullptr, int scan_limit = 0) {
    const int n = (int)jobs.size(), np = (int)passes_out.size();
    Carve in{align_up(sizeof(JpegDesc) * (size_t)n * np, 256)}, work{align_up(4 * (size_t)n, 256)}, coef;
    int max_groups = 1, max_seg = 1, max_blocks = 1, max_h = 1, max_w = 1;                // max_h, max_w: at full scale
    // A progressive file's scans (the first scan_limit of them) in launches by level: a scan waits for the earlier scans that hold one of
    // its components and overlap its band, and for no other -- scans of one level write different coefficients, each as 16-bit stores --
    // so libjpeg's ten-scan script is three launches: every first scan, then the refinements, then luma's last one.
    auto scans_of = [&](const FileJob& j) { return !j.prog ? 0 : (scan_limit > 0 ? std::min(scan_limit, j.prog->plan.n_scans) : j.prog->plan.n_scans); };
    struct LevelScan { int job, k; };
    std::vector<std::vector<LevelScan>> levels;
    size_t total_scans = 0;
    for (int i = 0; i < n; ++i) {
        const FileJob& j = jobs[i];
        std::vector<int> level((size_t)scans_of(j), 0);
        for (int k = 0; k < scans_of(j); ++k) {
            const bbocr_jpeg_scan& b = j.prog->plan.scans[k];
            for (int e = 0; e < k; ++e) {
                const bbocr_jpeg_scan& a = j.prog->plan.scans[e];
                bool shares = false;
                for (int x = 0; x < a.components; ++x)
                    for (int y = 0; y < b.components; ++y) shares |= a.component[x] == b.component[y];
                if (shares && a.ss <= b.se && b.ss <= a.se) level[k] = std::max(level[k], level[e] + 1);
            }
            if (levels.size() <= (size_t)level[k]) levels.resize((size_t)level[k] + 1);
            levels[level[k]].push_back({i, k});
            ++total_scans;
        }
    }
    std::vector<int> level_groups(levels.size(), 1);
    int prog_groups = 1, prog_max_seg = 1;                                    // of the first scans: workgroups of 64 subsequences, segments
    const size_t o_scans = in.add(sizeof(JpScan) * std::max<size_t>(total_scans, 1));
    for (FileJob& j : jobs) {
        const bbocr_jpeg_plan& pl = j.ps.plan;
        j.scan_blob.resize((size_t)scans_of(j));
        for (int k = 0; k < scans_of(j); ++k) {
            const bbocr_jpeg_scan& sc = j.prog->plan.scans[k];
            FileJob::ScanBlob& b = j.scan_blob[k];
            b = {};
            b.o_data = in.add((size_t)sc.bytes + 8);
            b.o_segbyte = in.add(4 * ((size_t)sc.segments + 1));
            b.o_huff = in.add(std::max<size_t>(prog_scan_tables(sc), 1) * sizeof(JpegHuff));
            b.subs = prog_scan_subs(sc, S);
            if (b.subs) {                                                     // a first scan: subsequence lists and states, as for a baseline scan
                b.o_segsub = in.add(4 * ((size_t)sc.segments + 1));
                b.o_subseg = in.add(4 * b.subs);
                b.w_entry = work.add(8 * b.subs);
                b.w_exits = work.add(8 * b.subs);
                b.w_count = work.add(4 * b.subs);
                b.w_scan = work.add(4 * b.subs);
                prog_groups = std::max(prog_groups, (int)((b.subs + 63) / 64));
            }
            prog_max_seg = std::max(prog_max_seg, sc.segments);
        }
        j.o_huff = in.add(4 * sizeof(JpegHuff));
        j.o_quant = in.add(3 * 64 * 2);
        j.o_segbyte = in.add(4 * ((size_t)pl.segments + 1));
        j.o_segsub = in.add(4 * ((size_t)pl.segments + 1));
        j.o_data = in.add((size_t)pl.scan_bytes + 8);
        // subsequences: every segment is cut on its own, so at most one per segment more than scan bits / S
        j.o_subseg = in.add(4 * ((size_t)pl.segments + (size_t)pl.scan_bytes * 8 / S + 1));
        j.nblocks = pl.mcu_cols * pl.mcu_rows * (pl.components == 3 ? luma_h(pl) * luma_v(pl) + 2 : 1);
        max_seg = std::max(max_seg, pl.segments);
        max_blocks = std::max(max_blocks, j.nblocks);
        max_h = std::max(max_h, pl.height);
        max_w = std::max(max_w, pl.width);
    }
    root->jd_pin.ensure(in.off);
    root->jd_in.ensure(in.off);
    char* hb = (char*)root->jd_pin.p;
    char* db = (char*)root->jd_in.p;
    for (FileJob& j : jobs) {                                             // fill the blob: unstuff, cut, derive
        const bbocr_jpeg_plan& pl = j.ps.plan;
        JpegHuff* ht = (JpegHuff*)(hb + j.o_huff);
        for (int cls = 0; cls < 2; ++cls)
            for (int id = 0; id < 2; ++id)
                if (!derive_table(j.ps.huff[cls][id], ht[cls * 2 + id])) std::memset(&ht[cls * 2 + id], 0, sizeof(JpegHuff));   // no code: the file fails
        std::memcpy(hb + j.o_quant, j.ps.quant, sizeof j.ps.quant);
        int* seg_byte = (int*)(hb + j.o_segbyte);
        int* seg_sub = (int*)(hb + j.o_segsub);
        int* sub_seg = (int*)(hb + j.o_subseg);
        uint8_t* data = (uint8_t*)(hb + j.o_data);
        size_t w = 0;
        int nsub = 0;
        for (int s = 0; s < pl.segments; ++s) {
            const uint8_t* a = j.file + j.ps.segs[s].first;
            const uint8_t* e = j.file + j.ps.segs[s].second;
            seg_byte[s] = (int)w;
            seg_sub[s] = nsub;
            w += unstuff(a, e, data + w);
            const size_t bits = (w - (size_t)seg_byte[s]) * 8;
            const int cnt = (int)std::max<size_t>((bits + S - 1) / S, 1);
            for (int k = 0; k < cnt; ++k) sub_seg[nsub + k] = s;
            nsub += cnt;
        }
        seg_byte[pl.segments] = (int)w;
        seg_sub[pl.segments] = nsub;
        j.data_bytes = w;
        j.nsub = nsub;
        j.groups = (nsub + JD_LANES - 1) / JD_LANES;
        max_groups = std::max(max_groups, j.groups);
        j.w_entry = work.add(8 * (size_t)nsub);
        j.w_exits = work.add(8 * (size_t)nsub);
        j.w_count = work.add(4 * (size_t)nsub);
        j.w_scan = work.add(4 * (size_t)nsub);
        j.w_first = work.add(4 * (size_t)nsub);
        for (int p = 0; p < np; ++p) {
            j.geo[p] = jpeg_geometry(pl, passes_out[p].scale);
            for (int c = 0; c < 3; ++c) j.w_plane[p][c] = work.add(plane_size(j.geo[p].comp[c]));
        }
        j.o_coef = coef.add((size_t)j.nblocks * 128);
    }
    const int passes = max_groups + 1;
    const size_t flags_off = work.off;
    for (FileJob& j : jobs) j.w_flags = work.add(4 * (size_t)passes);
    const int prog_passes = prog_groups + 1;
    for (FileJob& j : jobs)
        for (FileJob::ScanBlob& b : j.scan_blob)
            if (b.subs) b.w_flags = work.add(4 * (size_t)prog_passes);
    root->jd_work.ensure(work.off);
    root->jd_coef.ensure(std::max<size_t>(coef.off, 256));
    char* wb = (char*)root->jd_work.p;
    JpegDesc* descs = (JpegDesc*)hb;
    for (int k = 0; k < n; ++k) {
        const FileJob& j = jobs[k];
        const bbocr_jpeg_plan& pl = j.ps.plan;
        JpegDesc d{};
        d.data = (const uint8_t*)(db + j.o_data);
        d.seg_byte = (const int*)(db + j.o_segbyte);
        d.seg_sub = (const int*)(db + j.o_segsub);
        d.sub_seg = (const int*)(db + j.o_subseg);
        d.entry = (unsigned long long*)(wb + j.w_entry);
        d.exits = (unsigned long long*)(wb + j.w_exits);
        d.count = (int*)(wb + j.w_count);
        d.scan = (int*)(wb + j.w_scan);
        d.first = (int*)(wb + j.w_first);
        d.flags = (int*)(wb + j.w_flags);
        d.status = (int*)wb + k;
        d.coef = (short*)((char*)root->jd_coef.p + j.o_coef);
        d.huff = (const JpegHuff*)(db + j.o_huff);
        d.quant = (const unsigned short*)(db + j.o_quant);
        d.W = pl.width;
        d.H = pl.height;
        d.ncomp = pl.components;
        d.hs = luma_h(pl);
        d.vs = luma_v(pl);
        d.bpm = pl.components == 3 ? d.hs * d.vs + 2 : 1;
        d.mcux = pl.mcu_cols;
        d.mcuy = pl.mcu_rows;
        d.nmcu = pl.mcu_cols * pl.mcu_rows;
        d.ri = pl.restart_interval ? pl.restart_interval : d.nmcu;
        d.nseg = pl.segments;
        d.nsub = j.nsub;
        d.S = S;
        d.nblocks = j.nblocks;
        d.passes = passes;
        for (int c = 0; c < 3; ++c) { d.tab_dc[c] = j.ps.tab_dc[c]; d.tab_ac[c] = j.ps.tab_ac[c]; }
        for (int p = 0; p < np; ++p) {                                    // pass p's descriptors: descs[p * n ..]; the entropy stages read pass 0's
            for (int c = 0; c < 3; ++c) {
                d.plane[c] = (uint8_t*)(wb + j.w_plane[p][c]);
                d.comp[c] = j.geo[p].comp[c];
            }
            d.OW = j.geo[p].OW;
            d.OH = j.geo[p].OH;
            d.out = j.out[p];
            d.pitch = j.pitch[p];
            d.px = pl.components == 3 ? passes_out[p].px : 1;
            descs[(size_t)p * n + k] = d;
        }
    }
    JpScan* scans = (JpScan*)(hb + o_scans);
    std::memset(scans, 0, sizeof(JpScan) * std::max<size_t>(total_scans, 1));
    {
        size_t at = 0;
        for (size_t L = 0; L < levels.size(); ++L)
            for (const LevelScan& e : levels[L]) {
                const FileJob& j = jobs[e.job];
                const FileJob::ScanBlob& b = j.scan_blob[e.k];
                JpScan& sc = scans[at++];
                prog_fill_scan(*j.prog, e.k, j.file, S, (uint8_t*)(hb + b.o_data), (int*)(hb + b.o_segbyte), (JpegHuff*)(hb + b.o_huff),
                               (int*)(hb + b.o_segsub), (int*)(hb + b.o_subseg), sc);
                if (b.subs) {
                    sc.seg_sub = (const int*)(db + b.o_segsub);
                    sc.sub_seg = (const int*)(db + b.o_subseg);
                    sc.entry = (unsigned long long*)(wb + b.w_entry);
                    sc.exits = (unsigned long long*)(wb + b.w_exits);
                    sc.count = (int*)(wb + b.w_count);
                    sc.scan = (int*)(wb + b.w_scan);
                    sc.flags = (int*)(wb + b.w_flags);
                    sc.passes = prog_passes;
                }
                sc.data = (const uint8_t*)(db + b.o_data);
                sc.seg_byte = (const int*)(db + b.o_segbyte);
                sc.huff = (const JpegHuff*)(db + b.o_huff);
                sc.coef = descs[e.job].coef;
                sc.status = descs[e.job].status;
                level_groups[L] = std::max(level_groups[L], jp_scan_groups(sc.Ss, sc.Ah, sc.nseg, sc.nunits));
            }
    }
    if (descs_out) descs_out->assign(descs, descs + n);
    HIPCHK(hipMemcpyAsync(db, hb, in.off, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(wb, 0, align_up(4 * (size_t)n, 256), st));                    // status words
    HIPCHK(hipMemsetAsync(wb + flags_off, 0, work.off - flags_off, st));                // pass flags
    HIPCHK(hipMemsetAsync(root->jd_coef.p, 0, std::max<size_t>(coef.off, 256), st));
    const JpegDesc* dd = (const JpegDesc*)db;
    for (int pass = 0; pass < passes; ++pass) HIPCHK(launch_jd_sync(dd, n, max_groups, pass, st));
    HIPCHK(launch_jd_scan(dd, n, st));
    HIPCHK(launch_jd_write(dd, n, max_groups, st));
    HIPCHK(launch_jd_dc(dd, n, max_seg, st));
    {
        size_t at = 0;
        for (size_t L = 0; L < levels.size(); at += levels[L].size(), ++L)
            for (size_t c = 0; c < levels[L].size(); c += 32768) {        // a launch holds at most 65535 scans (the grid's second dimension)
                HIPCHK(launch_jp_first((const JpScan*)(db + o_scans) + at + c, (int)std::min<size_t>(levels[L].size() - c, 32768), prog_groups,
                                       prog_passes, prog_max_seg, st));
                HIPCHK(launch_jp_scan((const JpScan*)(db + o_scans) + at + c, (int)std::min<size_t>(levels[L].size() - c, 32768), level_groups[L], st));
            }
    }
    for (int p = 0; p < np; ++p) {
        const JpegDesc* dp = dd + (size_t)p * n;
        HIPCHK(launch_jd_idct(dp, n, max_blocks, st));
        HIPCHK(launch_jd_output(dp, n, scaled_dim(max_h, passes_out[p].scale), scaled_dim(max_w, passes_out[p].scale), st));
    }
    root->jd_count[0] += n;
    root->jd_count[1] += n;
    root->jd_count[2] += (long long)n * np;
    root->jd_count[3] += (long long)n * np;
    dev_status.assign((size_t)n, 0);
    HIPCHK(hipMemcpyAsync(dev_status.data(), wb, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
}

// The pixel entry points' body on the JPEG lane's stream: one entropy pass over the batch, then one IDCT + output pass per entry of
// outputs[0 .. n_outputs).  An output of the imread form is decoded un-oriented into jd_page -- Pillow's padded pixels (a dword per pixel)
// or the grey samples, tight rows -- and page_orient writes the caller's BGR page from there.  chroma_classes false: only the files the
// plan supports, 4:2:0 and grey.  Argument errors are raised before anything is queued; a refused file's destinations are never written.
void jpeg_decode_outputs(bbocr_ctx* ctx, hipStream_t st, const uint8_t* const* files, const size_t* bytes, int n, int layout,
                         const bbocr_jpeg_output* outputs, int n_outputs, int* status, bool chroma_classes, bool progressive = false) {
    if (!files || !bytes || !outputs || !status || n < 1) fail(BBOCR_ERR_ARG, "bad decode arguments");
    if (layout != BBOCR_PAGE_YCBCR3 && layout != BBOCR_PAGE_YCBCR4) fail(BBOCR_ERR_ARG, "layout must be BBOCR_PAGE_YCBCR3 or BBOCR_PAGE_YCBCR4");
    if (n_outputs < 1 || n_outputs > kMaxPasses) fail(BBOCR_ERR_ARG, "1 .. 4 outputs, one per scale");
    int imread = -1;                                                      // the output of the imread form
    for (int o = 0; o < n_outputs; ++o) {
        const bbocr_jpeg_output& O = outputs[o];
        if (!O.dev_out || !O.pitches || !jpeg_scale_ok(O.scale)) fail(BBOCR_ERR_ARG, "an output needs destinations, pitches and a scale of 1, 2, 4 or 8");
        if (O.form != BBOCR_JPEG_FORM_YCBCR && O.form != BBOCR_JPEG_FORM_IMREAD) fail(BBOCR_ERR_ARG, "unknown output form");
        if (O.form == BBOCR_JPEG_FORM_IMREAD && O.scale != 1) fail(BBOCR_ERR_ARG, "the imread form exists at scale 1 only");
        for (int q = 0; q < o; ++q)
            if (outputs[q].scale == O.scale) fail(BBOCR_ERR_ARG, "a scale is named twice");
        if (O.form == BBOCR_JPEG_FORM_IMREAD) imread = o;
    }
    auto decoded = [](const bbocr_jpeg_plan& pl) { return pl.components == 3 ? PAGE_YCC4 : PAGE_GRAY; };
    Carve pages;
    std::vector<FileJob> jobs = jpeg_admit(files, bytes, n, status, [&](FileJob& j) {
        const bbocr_jpeg_plan& pl = j.ps.plan;
        for (int o = 0; o < n_outputs; ++o) {
            const bbocr_jpeg_output& O = outputs[o];
            if (!O.dev_out[j.k]) return false;
            if (o == imread) {
                if (O.pitches[j.k] < (long long)page_px_bytes(PAGE_BGR) * (pl.orientation >= 5 ? pl.height : pl.width)) return false;
                j.pitch[o] = (long long)pl.width * page_px_bytes(decoded(pl));
            } else {
                if (O.pitches[j.k] < (long long)scaled_dim(pl.width, O.scale) * page_px_bytes(pl.components == 3 ? layout : PAGE_GRAY)) return false;
                j.out[o] = O.dev_out[j.k];
                j.pitch[o] = O.pitches[j.k];
            }
        }
        if (imread >= 0) j.o_page = pages.add((size_t)j.pitch[imread] * (size_t)pl.height);
        return true;
    }, chroma_classes, progressive);
    if (jobs.empty()) return;
    std::vector<JpegPass> passes;
    for (int o = 0; o < n_outputs; ++o) passes.push_back({outputs[o].scale, page_px_bytes(o == imread ? (int)PAGE_YCC4 : layout)});
    if (imread >= 0) {
        ctx->jd_page.ensure(pages.off);
        for (FileJob& j : jobs) j.out[imread] = Carve::at<uint8_t>(ctx->jd_page.p, j.o_page);
    }
    std::vector<int> ds;
    jpeg_run(ctx, st, jobs, JD_SUBSEQ_BITS, passes, ds);
    jpeg_report(jobs, ds, status);
    if (imread < 0) return;
    for (size_t i = 0; i < jobs.size(); ++i) {
        const FileJob& j = jobs[i];
        const bbocr_jpeg_plan& pl = j.ps.plan;
        if (ds[i]) continue;
        HIPCHK(launch_page_orient(j.out[imread], pl.height, pl.width, (size_t)j.pitch[imread], decoded(pl), pl.orientation, PAGE_BGR,
                                  outputs[imread].dev_out[j.k], (size_t)outputs[imread].pitches[j.k], st));
    }
    HIPCHK(hipStreamSynchronize(st));
}

// The stage entry points' body: ONE file decoded at `scale` with S-bit subsequences, then stage 2 = the component planes in
// jpeg_geometry's sizes, Y, Cb, Cr one after the other, or stage 3 = the pixels, tight, copied to dev_dst.  cls: the files it takes -- -1
// every file the decoder takes, 0 the 4:2:0 and grey ones only, 1 those of a chroma class only.  Returns the file's descriptor (the
// entropy stages' intermediates).
JpegDesc jpeg_stage_run(bbocr_ctx* ctx, hipStream_t s, int stage, const uint8_t* file, size_t bytes, int S, int scale, int cls, void* dev_dst,
                        size_t dst_bytes, int* file_status, bool progressive = false, int scan_limit = 0) {
    if (!file || !dev_dst || stage < 0 || stage > 3 || bytes >= ((size_t)1 << 28)) fail(BBOCR_ERR_ARG, "bad stage arguments");
    int status = 0;
    std::vector<FileJob> jobs = jpeg_admit(&file, &bytes, 1, &status, [&](FileJob& j) {
        const bbocr_jpeg_plan& pl = j.ps.plan;
        if (cls >= 0 && cls != (pl.chroma != 0)) return false;
        const JpegGeometry g = jpeg_geometry(pl, scale);
        const size_t pix = (size_t)g.OW * g.OH * pl.components;
        const size_t planes = plane_size(g.comp[0]) + plane_size(g.comp[1]) + plane_size(g.comp[2]);
        if ((stage == 3 && dst_bytes < pix) || (stage == 2 && dst_bytes < planes)) fail(BBOCR_ERR_ARG, "destination too small");
        ctx->jd_stage.ensure(pix);                               // the pixels go to a scratch image unless they are the stage's output
        j.out[0] = stage == 3 ? (uint8_t*)dev_dst : (uint8_t*)ctx->jd_stage.p;
        j.pitch[0] = (long long)g.OW * pl.components;
        return true;
    }, true, progressive);
    if (jobs.empty()) fail(BBOCR_ERR_ARG, "the plan refuses this file, or this entry point does not take its sampling");
    std::vector<int> ds;
    std::vector<JpegDesc> descs;
    jpeg_run(ctx, s, jobs, S, {{scale, 3}}, ds, &descs, scan_limit);
    jpeg_report(jobs, ds, &status);
    if (file_status) *file_status = status;
    const JpegDesc& d = descs[0];
    size_t off = 0;
    for (int c = 0; stage == 2 && c < d.ncomp; ++c) {
        HIPCHK(hipMemcpyAsync((char*)dev_dst + off, d.plane[c], plane_size(d.comp[c]), hipMemcpyDeviceToDevice, s));
        off += plane_size(d.comp[c]);
    }
    HIPCHK(hipStreamSynchronize(s));
    return d;
}

bool draft_scale(int s) { return s == 2 || s == 4 || s == 8; }

}  // namespace

extern "C" {

int bbocr_host_jpeg_plan(const uint8_t* file, size_t bytes, bbocr_jpeg_plan* plan) {
    if (!file || !plan) return BBOCR_ERR_ARG;
    JpegParsed ps;
    const int reason = jpeg_parse(file, bytes, ps, false);
    *plan = ps.plan;
    plan->reason = reason;
    return BBOCR_OK;
}

int bbocr_jpeg_decode_scaled(bbocr_ctx* ctx, const uint8_t* const* files, const size_t* bytes, int n, int layout, int scale,
                             uint8_t* const* dev_out, const long long* pitches, int* status) {
    return lane_guarded(ctx, &bbocr_ctx::jpeg_lane, true, [&](hipStream_t st) {
        const bbocr_jpeg_output out{scale, BBOCR_JPEG_FORM_YCBCR, dev_out, pitches};
        jpeg_decode_outputs(ctx, st, files, bytes, n, layout, &out, 1, status, scale == 1);
    });
}

int bbocr_jpeg_decode(bbocr_ctx* ctx, const uint8_t* const* files, const size_t* bytes, int n, int layout, uint8_t* const* dev_out,
                      const long long* pitches, int* status) {
    return bbocr_jpeg_decode_scaled(ctx, files, bytes, n, layout, 1, dev_out, pitches, status);
}

int bbocr_jpeg_scaled_dims(int H, int W, int scale, int* out_h, int* out_w) {
    if (H < 1 || W < 1 || !jpeg_scale_ok(scale) || !out_h || !out_w) return BBOCR_ERR_ARG;
    *out_h = scaled_dim(H, scale);
    *out_w = scaled_dim(W, scale);
    return BBOCR_OK;
}

int bbocr_jpeg_imread(bbocr_ctx* ctx, const uint8_t* const* files, const size_t* bytes, int n, uint8_t* const* dev_out, const long long* pitches,
                      int* status) {
    return lane_guarded(ctx, &bbocr_ctx::jpeg_lane, true, [&](hipStream_t st) {
        const bbocr_jpeg_output out{1, BBOCR_JPEG_FORM_IMREAD, dev_out, pitches};
        jpeg_decode_outputs(ctx, st, files, bytes, n, BBOCR_PAGE_YCBCR4, &out, 1, status, true);   // the layout: of YCbCr outputs, here none
    });
}

int bbocr_jpeg_decode_scales(bbocr_ctx* ctx, const uint8_t* const* files, const size_t* bytes, int n, int layout, const bbocr_jpeg_output* outputs,
                             int n_outputs, int* status) {
    return lane_guarded(ctx, &bbocr_ctx::jpeg_lane, true,
                        [&](hipStream_t st) { jpeg_decode_outputs(ctx, st, files, bytes, n, layout, outputs, n_outputs, status, true); });
}

int bbocr_host_jpeg_progressive_plan(const uint8_t* file, size_t bytes, bbocr_jpeg_progressive_plan* plan) {
    if (!file || !plan) return BBOCR_ERR_ARG;
    ProgParsed pp;
    prog_parse(file, bytes, pp, false);
    *plan = pp.plan;
    return BBOCR_OK;
}

int bbocr_jpeg_decode_progressive(bbocr_ctx* ctx, const uint8_t* const* files, const size_t* bytes, int n, int layout,
                                  const bbocr_jpeg_output* outputs, int n_outputs, int* status) {
    return lane_guarded(ctx, &bbocr_ctx::jpeg_lane, true,
                        [&](hipStream_t st) { jpeg_decode_outputs(ctx, st, files, bytes, n, layout, outputs, n_outputs, status, true, true); });
}

int bbocr_op_jpeg_progressive_stage(bbocr_ctx* ctx, int stage, const uint8_t* file, size_t bytes, int n_scans, int subseq_bits, void* dev_dst,
                                    size_t dst_bytes, int* file_status) {
    return lane_guarded(ctx, &bbocr_ctx::jpeg_lane, true, [&](hipStream_t s) {
        const int S = subseq_bits == 0 ? JD_SUBSEQ_BITS : subseq_bits;
        if (S < 32 || S > 65536 || (S & 7)) fail(BBOCR_ERR_ARG, "subseq_bits: a multiple of 8 in 32 .. 65536, or 0");
        if (stage < 1 || stage > 3 || n_scans < 0 || n_scans > BBOCR_JPEG_MAX_SCANS) fail(BBOCR_ERR_ARG, "stage 1, 2 or 3 after 0 .. 64 scans");
        const JpegDesc d = jpeg_stage_run(ctx, s, stage, file, bytes, S, 1, -1, dev_dst, dst_bytes, file_status, true, n_scans);
        if (stage == 1) {
            if (dst_bytes < (size_t)d.nblocks * 128) fail(BBOCR_ERR_ARG, "destination too small");
            HIPCHK(hipMemcpyAsync(dev_dst, d.coef, (size_t)d.nblocks * 128, hipMemcpyDeviceToDevice, s));
        }
        HIPCHK(hipStreamSynchronize(s));
    });
}

int bbocr_op_jpeg_stage(bbocr_ctx* ctx, int stage, const uint8_t* file, size_t bytes, int subseq_bits, void* dev_dst, size_t dst_bytes,
                        int* file_status) {
    return lane_guarded(ctx, &bbocr_ctx::jpeg_lane, true, [&](hipStream_t s) {
        const int S = subseq_bits == 0 ? JD_SUBSEQ_BITS : subseq_bits;
        if (S < 32 || S > 65536 || (S & 7)) fail(BBOCR_ERR_ARG, "subseq_bits: a multiple of 8 in 32 .. 65536, or 0");
        const JpegDesc d = jpeg_stage_run(ctx, s, stage, file, bytes, S, 1, -1, dev_dst, dst_bytes, file_status);
        if (stage == 0) {
            const size_t ns = (size_t)d.nsub;
            if (dst_bytes < ns * 16) fail(BBOCR_ERR_ARG, "destination too small");
            std::vector<unsigned long long> entry(ns);
            std::vector<int> first(ns), rows(ns * 4);
            HIPCHK(hipMemcpyAsync(entry.data(), d.entry, ns * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(first.data(), d.first, ns * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            for (size_t i = 0; i < ns; ++i) {
                rows[4 * i] = (int)(unsigned)entry[i];
                rows[4 * i + 1] = (int)((entry[i] >> 32) & 7);
                rows[4 * i + 2] = (int)((entry[i] >> 40) & 63);
                rows[4 * i + 3] = first[i];
            }
            HIPCHK(hipMemcpyAsync(dev_dst, rows.data(), ns * 16, hipMemcpyHostToDevice, s));
        } else if (stage == 1) {
            if (dst_bytes < (size_t)d.nblocks * 128) fail(BBOCR_ERR_ARG, "destination too small");
            HIPCHK(hipMemcpyAsync(dev_dst, d.coef, (size_t)d.nblocks * 128, hipMemcpyDeviceToDevice, s));
        }
        HIPCHK(hipStreamSynchronize(s));
    });
}

int bbocr_op_jpeg_scaled_stage(bbocr_ctx* ctx, int stage, const uint8_t* file, size_t bytes, int scale, void* dev_dst, size_t dst_bytes,
                               int* file_status) {
    return lane_guarded(ctx, &bbocr_ctx::jpeg_lane, true, [&](hipStream_t s) {
        if ((stage != 2 && stage != 3) || !draft_scale(scale)) fail(BBOCR_ERR_ARG, "stage 2 or 3 at scale 2, 4 or 8");
        jpeg_stage_run(ctx, s, stage, file, bytes, JD_SUBSEQ_BITS, scale, 0, dev_dst, dst_bytes, file_status);
    });
}

int bbocr_op_jpeg_scaled_class_stage(bbocr_ctx* ctx, int stage, const uint8_t* file, size_t bytes, int scale, void* dev_dst, size_t dst_bytes,
                                     int* file_status) {
    return lane_guarded(ctx, &bbocr_ctx::jpeg_lane, true, [&](hipStream_t s) {
        if ((stage != 2 && stage != 3) || !draft_scale(scale)) fail(BBOCR_ERR_ARG, "stage 2 or 3 at scale 2, 4 or 8");
        jpeg_stage_run(ctx, s, stage, file, bytes, JD_SUBSEQ_BITS, scale, 1, dev_dst, dst_bytes, file_status);
    });
}

int bbocr_jpeg_counters(bbocr_ctx* ctx, long long* out) {
    return status_of(ctx, [&] {
        if (!out) fail(BBOCR_ERR_ARG, "bad counter arguments");
        std::lock_guard<std::mutex> lk(ctx->jpeg_lane.mu);
        std::memcpy(out, ctx->jd_count, sizeof ctx->jd_count);
    });
}

int bbocr_host_jpeg_scaled_geometry(const bbocr_jpeg_plan* plan, int scale, bbocr_jpeg_scaled_comp* comps) {
    if (!plan || !comps || !draft_scale(scale) || !jpeg_taken(*plan)) return BBOCR_ERR_ARG;
    if ((plan->components != 1 && plan->components != 3) || plan->mcu_cols < 1 || plan->mcu_rows < 1) return BBOCR_ERR_ARG;
    const JpegGeometry g = jpeg_geometry(*plan, scale);
    for (int c = 0; c < 3; ++c) {                                         // comps[components .. 3) come out zeroed
        const JpegComp& k = g.comp[c];
        comps[c] = {k.n, k.plane_rows, k.pitch, k.valid_rows, k.valid_cols, k.up};
    }
    return BBOCR_OK;
}

}  // extern "C"
