// JPEG decoding, host side: the per-batch tables of jpegdec.hip and jpegprog.hip (unstuffed segment bytes and subsequence lists from
// jpeg_parse.h's cut_scan, carved and bound by ScanOffsets for a baseline scan and a progressive one alike; derived Huffman tables) and
// the launch sequence.  The marker walks behind bbocr_host_jpeg_plan and bbocr_host_jpeg_progressive_plan are jpeg_parse.h's.  A batch runs on
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

// Where a scan that cut_scan cuts lies: its tables in the input blob, the states of its subsequences in the work buffer.  subs: the
// subsequences the blob has room for; 0: the scan is not cut (a refinement) and has its bytes and seg_byte alone.
struct ScanOffsets {
    size_t data, seg_byte, seg_sub, sub_seg, subs, entry, exits, count, scan, flags;
    void blob(Carve& in, int segments, long long bytes, size_t room) {
        *this = {};
        subs = room;
        data = in.add((size_t)bytes + 8);
        seg_byte = in.add(4 * ((size_t)segments + 1));
        if (!subs) return;
        seg_sub = in.add(4 * ((size_t)segments + 1));
        sub_seg = in.add(4 * subs);
    }
    void states(Carve& work, size_t nsub) {
        entry = work.add(8 * nsub);
        exits = work.add(8 * nsub);
        count = work.add(4 * nsub);
        scan = work.add(4 * nsub);
    }
    // the descriptor's pointers into the device's copy of the blob (db) and the work buffer (wb)
    void bind(char* db, char* wb, int passes, JpegSubs& d) const {
        d.data = (const uint8_t*)(db + data);
        d.seg_byte = (const int*)(db + seg_byte);
        if (!subs) return;
        d.seg_sub = (const int*)(db + seg_sub);
        d.sub_seg = (const int*)(db + sub_seg);
        d.entry = (unsigned long long*)(wb + entry);
        d.exits = (unsigned long long*)(wb + exits);
        d.count = (int*)(wb + count);
        d.scan = (int*)(wb + scan);
        d.flags = (int*)(wb + flags);
        d.passes = passes;
    }
};

struct FileJob {                              // one admitted file of a batch
    JpegParsed ps;
    const uint8_t* file = nullptr;            // its bytes (caller-owned)
    uint8_t* out[kMaxPasses] = {nullptr};     // per pass: where the decoder writes its pixels, rows `pitch` bytes apart
    long long pitch[kMaxPasses] = {0};
    int k = 0;                                // its index in the caller's arrays (status[])
    int nsub = 0, groups = 0, nblocks = 0;
    ScanOffsets cut;                          // its scan (a progressive file: no segment, no byte)
    size_t o_huff, o_quant;                   // offsets in the input blob
    size_t w_first, w_plane[kMaxPasses][3], o_coef; // offsets in the work / coefficient buffers
    size_t o_page = 0;                        // the imread form: offset of the un-oriented decode in jd_page
    JpegGeometry geo[kMaxPasses];             // per pass (filled by jpeg_run)
    std::shared_ptr<ProgParsed> prog;         // a progressive file: its scans; `ps` then holds the frame alone, as a plan without a scan
    struct ScanBlob { ScanOffsets cut; size_t o_huff; };
    std::vector<ScanBlob> scan_blob;          // per scan of a progressive file
};

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
            j.ps = j.prog->frame;                                                       // a plan without a scan
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
            b.cut.blob(in, sc.segments, sc.bytes, prog_scan_subs(sc, S));
            b.o_huff = in.add(std::max<size_t>(prog_scan_tables(sc), 1) * sizeof(JpegHuff));
            if (b.cut.subs) {                                                 // a first scan: states as for a baseline scan
                b.cut.states(work, b.cut.subs);
                prog_groups = std::max(prog_groups, (int)((b.cut.subs + 63) / 64));
            }
            prog_max_seg = std::max(prog_max_seg, sc.segments);
        }
        j.o_huff = in.add(4 * sizeof(JpegHuff));
        j.o_quant = in.add(3 * 64 * 2);
        j.cut.blob(in, pl.segments, pl.scan_bytes, scan_subs_bound(pl.segments, pl.scan_bytes, S));
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
        const ScanOffsets& o = j.cut;
        cut_scan(j.file, j.ps.segs, S, (uint8_t*)(hb + o.data), (int*)(hb + o.seg_byte), (int*)(hb + o.seg_sub), (int*)(hb + o.sub_seg), j.nsub);
        j.groups = (j.nsub + JD_LANES - 1) / JD_LANES;
        max_groups = std::max(max_groups, j.groups);
        j.cut.states(work, (size_t)j.nsub);
        j.w_first = work.add(4 * (size_t)j.nsub);
        for (int p = 0; p < np; ++p) {
            j.geo[p] = jpeg_geometry(pl, passes_out[p].scale);
            for (int c = 0; c < 3; ++c) j.w_plane[p][c] = work.add(plane_size(j.geo[p].comp[c]));
        }
        j.o_coef = coef.add((size_t)j.nblocks * 128);
    }
    const int passes = max_groups + 1;
    const size_t flags_off = work.off;
    for (FileJob& j : jobs) j.cut.flags = work.add(4 * (size_t)passes);
    const int prog_passes = prog_groups + 1;
    for (FileJob& j : jobs)
        for (FileJob::ScanBlob& b : j.scan_blob)
            if (b.cut.subs) b.cut.flags = work.add(4 * (size_t)prog_passes);
    root->jd_work.ensure(work.off);
    root->jd_coef.ensure(std::max<size_t>(coef.off, 256));
    char* wb = (char*)root->jd_work.p;
    JpegDesc* descs = (JpegDesc*)hb;
    for (int k = 0; k < n; ++k) {
        const FileJob& j = jobs[k];
        const bbocr_jpeg_plan& pl = j.ps.plan;
        JpegDesc d{};
        j.cut.bind(db, wb, passes, d);
        d.first = (int*)(wb + j.w_first);
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
                const ScanOffsets& o = b.cut;
                JpScan& sc = scans[at++];
                prog_fill_scan(*j.prog, e.k, j.file, S, (uint8_t*)(hb + o.data), (int*)(hb + o.seg_byte), (JpegHuff*)(hb + b.o_huff),
                               (int*)(hb + o.seg_sub), (int*)(hb + o.sub_seg), sc);
                o.bind(db, wb, prog_passes, sc);
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
// entropy stages' intermediates); bits: receives the decoder's JD_ERR_* bits for the file.
JpegDesc jpeg_stage_run(bbocr_ctx* ctx, hipStream_t s, int stage, const uint8_t* file, size_t bytes, int S, int scale, int cls, void* dev_dst,
                        size_t dst_bytes, int* file_status, bool progressive = false, int scan_limit = 0, int* bits = nullptr) {
    if (!file || !dev_dst || stage < 0 || stage > 4 || bytes >= ((size_t)1 << 28)) fail(BBOCR_ERR_ARG, "bad stage arguments");
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
    if (bits) *bits = ds[0];
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

// bbocr_op_jpeg_stage and bbocr_op_jpeg_progressive_stage: the subsequence length they name, and their stage 1 (the coefficients)
int stage_subseq_bits(int subseq_bits) {
    const int S = subseq_bits == 0 ? JD_SUBSEQ_BITS : subseq_bits;
    if (S < 32 || S > 65536 || (S & 7)) fail(BBOCR_ERR_ARG, "subseq_bits: a multiple of 8 in 32 .. 65536, or 0");
    return S;
}
void stage_coefficients(const JpegDesc& d, void* dev_dst, size_t dst_bytes, hipStream_t s) {
    if (dst_bytes < (size_t)d.nblocks * 128) fail(BBOCR_ERR_ARG, "destination too small");
    HIPCHK(hipMemcpyAsync(dev_dst, d.coef, (size_t)d.nblocks * 128, hipMemcpyDeviceToDevice, s));
}

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
        const int S = stage_subseq_bits(subseq_bits);
        if (stage < 1 || stage > 3 || n_scans < 0 || n_scans > BBOCR_JPEG_MAX_SCANS) fail(BBOCR_ERR_ARG, "stage 1, 2 or 3 after 0 .. 64 scans");
        const JpegDesc d = jpeg_stage_run(ctx, s, stage, file, bytes, S, 1, -1, dev_dst, dst_bytes, file_status, true, n_scans);
        if (stage == 1) stage_coefficients(d, dev_dst, dst_bytes, s);
        HIPCHK(hipStreamSynchronize(s));
    });
}

int bbocr_op_jpeg_stage(bbocr_ctx* ctx, int stage, const uint8_t* file, size_t bytes, int subseq_bits, void* dev_dst, size_t dst_bytes,
                        int* file_status) {
    return lane_guarded(ctx, &bbocr_ctx::jpeg_lane, true, [&](hipStream_t s) {
        int bits = 0;
        const JpegDesc d = jpeg_stage_run(ctx, s, stage, file, bytes, stage_subseq_bits(subseq_bits), 1, -1, dev_dst, dst_bytes, file_status, false, 0, &bits);
        if (stage == 4) {
            if (dst_bytes < 4) fail(BBOCR_ERR_ARG, "destination too small");
            HIPCHK(hipMemcpyAsync(dev_dst, &bits, 4, hipMemcpyHostToDevice, s));
        } else if (stage == 0) {
            const size_t ns = (size_t)d.nsub;
            if (dst_bytes < ns * 16) fail(BBOCR_ERR_ARG, "destination too small");
            std::vector<unsigned long long> entry(ns);
            std::vector<int> first(ns), rows(ns * 4);
            HIPCHK(hipMemcpyAsync(entry.data(), d.entry, ns * 8, hipMemcpyDeviceToHost, s));
            HIPCHK(hipMemcpyAsync(first.data(), d.first, ns * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            for (size_t i = 0; i < ns; ++i) {
                const JpegState st = jpeg_unpack(entry[i]);
                rows[4 * i] = (int)st.p;
                rows[4 * i + 1] = st.b;
                rows[4 * i + 2] = st.z;
                rows[4 * i + 3] = first[i];
            }
            HIPCHK(hipMemcpyAsync(dev_dst, rows.data(), ns * 16, hipMemcpyHostToDevice, s));
        } else if (stage == 1) {
            stage_coefficients(d, dev_dst, dst_bytes, s);
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
