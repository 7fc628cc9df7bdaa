// Dictionary-constrained CTC decode: readtext(decoder='wordbeamsearch') over a caller's word list.
//
// Restates easyocr 1.7.2's CTCLabelConverter.decode_wordbeamsearch and easyocr/utils.py::ctcBeamSearch(mat, classes, ignore_idx, lm=None,
// beamWidth, dict_list) for a model WITHOUT separator characters -- every generation-2 model.  easyocr's sources are not part of this
// repository: as with ctc_beam.cpp, the host function here (ctc_wordbeam_host.h::ctc_wordbeam_search_host, over ctc_beam_host.h's step
// loop) IS the definition the device kernels (ctc_wordbeam.hip) are held to, text for text.
//
// For one sequence mat[T, C] -- the probabilities the CTC stage writes, after the ignore mask and the renormalisation:
//   1. Word groups.  a[t] = argmax_c mat[t][c], the lowest index among equals (what ctc_rows_kernel writes as idx).  `space` is the class of
//      ' ' (43 in english_g2).  Word groups are the maximal runs of consecutive t with a[t] != space.  Rows whose arg-max is the space belong
//      to no group and are read by no search.  A sequence of nothing but spaces has no group and decodes to the empty text.
//   2. Per group: ctc_beam_search_host's loop, unchanged, on the group's rows alone -- the threshold 0.5 / C with the blank a candidate,
//      float32 in the host's association, the stable ranking by total over the dictionary's insertion order, entries identified by their
//      labelling.
//   3. Candidate selection.  After the last step ALL entries of the final step's dictionary (the unpruned `curr`) are ranked by the same
//      stable rule and the first min(BBOCR_WORD_CANDIDATES, #entries) are the candidates (20: upstream's wordsearch(classes, ignore_idx, 20,
//      dict_list)).  Each is collapsed in rank order as ever -- class 0 dropped, and every symbol equal to its predecessor in the labelling.
//      The word is the first candidate whose collapsed text is an element of the dictionary; if none is, candidate 0 -- exactly what
//      'beamsearch' returns on those rows.  The empty text is never a member.
//   4. Join.  The sequence's text is the words joined by one `space` class; a word that collapsed to nothing still contributes its
//      separator (upstream's string += ' ' + t, the leading one stripped).  The result never exceeds T symbols: a word is at most its rows,
//      and groups are at least one space row apart -- so it fits the sequence's own rows of the row-indexed text buffer.
//   5. Boxes, box order and the confidence are the greedy path's (custom_mean of the rows' maxima), as for every decoder.
//
// A consequence: the collapse removes adjacent repeats from the LABELLING, and the blank is an ordinary symbol of a labelling.  The labelling
// that reads a doubled letter the CTC way -- (b, o, o, k), the second o entered through prBlank -- collapses to "bok"; only a labelling that
// holds the blank SYMBOL between the pair, (b, o, 0, o, k), collapses to "book".  So a word with a doubled letter is matched through such
// lower-ranked candidates only.  The quirk is upstream's and the beam search is already held to it; bbocr_dictionary_stats counts the words
// with a doubled letter when the list is loaded.
//
// This file: the batch over a {first row, T} table, the route rule, the context's dictionary, the device half of a pass, and the entry points.
#include "ctx.h"
#include "ctc_wordbeam_host.h"

void ctc_wordbeam_search_batch(const float* probs, const int* seqs, int nseq, int C, int cs, int beam_width, int space, const WdTable* dict,
                               std::vector<std::vector<int>>& texts, HostPool* pool) {
    texts.assign((size_t)nseq, {});
    auto one = [&](int i) {
        ctc_wordbeam_search_host(probs + (size_t)seqs[2 * i] * cs, seqs[2 * i + 1], C, cs, beam_width, space, dict, texts[i]);
    };
    if (pool) pool->parallel_for(nseq, one);
    else for (int i = 0; i < nseq; ++i) one(i);
}

// the device where its kernel takes the pass: at most 128 classes (labellings and dictionary symbols are bytes), a width the LDS block
// holds, and a longest SEQUENCE -- which bounds every word group -- whose block fits
int wordbeam_route(int beam_width, int C, const int* seqs, int nseq) {
    int max_T = 0;
    for (int i = 0; i < nseq; ++i) max_T = std::max(max_T, seqs[2 * i + 1]);
    return ctc_wordbeam_on_device(beam_width, C, max_T) ? CTC_WORD_DEVICE : CTC_WORD_HOST;
}

static int word_seg_cap(const int* seqs, int nseq) {
    long long cap = 0;
    for (int i = 0; i < nseq; ++i) cap += (std::max(seqs[2 * i + 1], 0) + 1) / 2;
    if (cap > INT32_MAX / 4) fail(BBOCR_ERR_ARG, "too many rows for one word search");
    return (int)std::max<long long>(cap, 1);
}

void wordbeam_device(bbocr_ctx* c, const float* probs_dev, const int* idx_dev, size_t rows, int C, int cs, const int* seqs, const int* seqs_dev, int nseq,
                     int beam_width, hipStream_t s) {
    if (!c->wd_dev.slots || !c->wd_host) fail(BBOCR_ERR_STATE, "no dictionary on the device");
    int max_T = 0;
    for (int i = 0; i < nseq; ++i) max_T = std::max(max_T, seqs[2 * i + 1]);
    const int cap = word_seg_cap(seqs, nseq);
    const size_t rows1 = std::max<size_t>(rows, 1);
    c->wb_segs.ensure((size_t)cap * 12);                         // {first row, T} x cap | length x cap
    c->wb_meta.ensure((size_t)nseq * 8 + 16);                    // {first segment, count} x nseq | the counter
    c->wb_text.ensure(rows1 * 4);
    c->ctc_beam_idx.ensure(rows1 * 4);
    c->ctc_beam_len.ensure((size_t)nseq * 4);
    int* segs = (int*)c->wb_segs.p;
    int* seg_len = segs + (size_t)cap * 2;
    int* seq_seg = (int*)c->wb_meta.p;
    int* counter = seq_seg + (size_t)nseq * 2;
    if (!idx_dev) {
        c->ctc_idx.ensure(rows1 * 4);
        HIPCHK(launch_row_argmax(probs_dev, rows, C, cs, (int*)c->ctc_idx.p, s));
        idx_dev = (const int*)c->ctc_idx.p;
    }
    HIPCHK(launch_word_segments(idx_dev, rows, seqs_dev, nseq, c->wd_host->space, segs, cap, seq_seg, counter, s));
    HIPCHK(launch_ctc_wordbeam(probs_dev, rows, C, cs, seqs_dev, nseq, max_T, beam_width, c->wd_host->space, c->wd_dev, segs, cap, seq_seg, counter, seg_len,
                               (int*)c->wb_text.p, (int*)c->ctc_beam_idx.p, (int*)c->ctc_beam_len.p, s));
}

// the table as the kernels read it: slots, then the pool narrowed to bytes -> buf (uploaded on s; the caller waits)
static WordDictDev upload_dict(const WdTable& t, DevBuf& buf, std::vector<unsigned char>& stage, hipStream_t s) {
    const size_t slot_bytes = t.slots.size() * sizeof(WdSlot);
    stage.assign(slot_bytes + t.pool.size(), 0);
    memcpy(stage.data(), t.slots.data(), slot_bytes);
    for (size_t i = 0; i < t.pool.size(); ++i) stage[slot_bytes + i] = (unsigned char)t.pool[i];
    buf.ensure(stage.size());
    HIPCHK(hipMemcpyAsync(buf.p, stage.data(), stage.size(), hipMemcpyHostToDevice, s));
    WordDictDev d;
    d.slots = buf.p;
    d.pool = (const unsigned char*)buf.p + slot_bytes;
    d.nslots = (unsigned int)t.slots.size();
    d.pool_n = (unsigned int)t.pool.size();
    d.probe = t.longest_probe;
    return d;
}

static void check_seqs(const int* seqs, int nseq, size_t rows, int& max_T) {
    max_T = 0;
    for (int i = 0; i < nseq; ++i) {
        const long long first = seqs[2 * i], T = seqs[2 * i + 1];
        if (first < 0 || T < 0 || first + T > (long long)rows) fail(BBOCR_ERR_ARG, "a sequence lies outside the rows");
        max_T = std::max(max_T, (int)T);
    }
}

extern "C" {

int bbocr_host_ctc_wordbeam(const float* probs, int n, int T, int C, int cs, int beam_width, int space_class, const uint16_t* symbols,
                            const int* word_off, int n_words, int* text_off, int* text_idx) {
    if (!probs || !text_off || !text_idx || n <= 0 || T <= 0 || C <= 0 || C > cs || beam_width <= 0 || space_class < 1 || space_class >= C || n_words < 0)
        return BBOCR_ERR_ARG;
    try {
        WdTable dict;
        if (!wd_build(symbols, word_off, n_words, C, space_class, 0, dict)) return BBOCR_ERR_ARG;
        std::vector<int> seqs;
        for (int i = 0; i < n; ++i) { seqs.push_back(i * T); seqs.push_back(T); }
        std::vector<std::vector<int>> texts;
        ctc_wordbeam_search_batch(probs, seqs.data(), n, C, cs, beam_width, space_class, &dict, texts);
        int o = 0;
        for (int i = 0; i < n; ++i) {
            text_off[i] = o;
            for (int v : texts[i]) text_idx[o++] = v;
        }
        text_off[n] = o;
    } catch (...) {
        return BBOCR_ERR_INTERNAL;
    }
    return BBOCR_OK;
}

int bbocr_host_wordbeam_route(int beam_width, int C, const int* seqs, int nseq) {
    if ((nseq > 0 && !seqs) || nseq < 0 || beam_width <= 0 || C <= 0) return BBOCR_ERR_ARG;
    return wordbeam_route(beam_width, C, seqs, nseq);
}

int bbocr_set_dictionary(bbocr_ctx* ctx, const uint16_t* symbols, const int* word_off, int n_words, int space_class) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        const int C = rec_classes(ctx);
        if (n_words == 0) {                     // cleared: decoder == WORDBEAMSEARCH is an argument error again
            ctx->wd_dev = WordDictDev();
            ctx->wd_host = nullptr;
            ctx->wd_table.reset();
            return;
        }
        if (space_class < 1 || space_class >= C) fail(BBOCR_ERR_ARG, "space_class: a class of the model other than the blank");
        auto t = std::make_unique<WdTable>();
        if (!wd_build(symbols, word_off, n_words, C, space_class, 0, *t))
            fail(BBOCR_ERR_ARG, "bad dictionary: every word needs 1 .. 1024 symbols, each a class in 1 .. C - 1 other than the space");
        WordDictDev d;
        if (C <= 128) {                         // every slot is leased: nothing reads the old table while the new one replaces it
            std::vector<unsigned char> stage;
            d = upload_dict(*t, ctx->wd_buf, stage, ctx->stream);
            slot_sync(ctx, ctx->stream);
        }
        ctx->wd_table = std::move(t);
        ctx->wd_host = ctx->wd_table.get();
        ctx->wd_dev = d;
    }, /*exclusive=*/true);
}

int bbocr_dictionary_stats(bbocr_ctx* ctx, int* words, int* slots, int* longest_probe, int* unmatchable) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        const WdTable* t = ctx->wd_host;
        if (words) *words = t ? t->words : 0;
        if (slots) *slots = t ? (int)t->slots.size() : 0;
        if (longest_probe) *longest_probe = t ? t->longest_probe : 0;
        if (unmatchable) *unmatchable = t ? t->unmatchable : 0;
    });
}

int bbocr_op_word_segments(bbocr_ctx* ctx, const int* dev_idx, size_t rows, const int* seqs, int nseq, int space_class, int* seg_off, int* segs) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        if (!dev_idx || !seqs || !seg_off || !segs || nseq <= 0 || rows > (size_t)INT32_MAX || space_class < 0) fail(BBOCR_ERR_ARG, "bad word-segment arguments");
        int max_T;
        check_seqs(seqs, nseq, rows, max_T);
        const int cap = word_seg_cap(seqs, nseq);
        ctx->seq_tables.ensure((size_t)nseq * 8);
        ctx->wb_segs.ensure((size_t)cap * 12);
        ctx->wb_meta.ensure((size_t)nseq * 8 + 16);
        int* seq_seg_dev = (int*)ctx->wb_meta.p;
        HIPCHK(hipMemcpyAsync(ctx->seq_tables.p, seqs, (size_t)nseq * 8, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(launch_word_segments(dev_idx, rows, (const int*)ctx->seq_tables.p, nseq, space_class, (int*)ctx->wb_segs.p, cap, seq_seg_dev,
                                    seq_seg_dev + (size_t)nseq * 2, ctx->stream));
        std::vector<int> tab((size_t)cap * 2), seq_seg((size_t)nseq * 2);
        int total = 0;
        HIPCHK(hipMemcpyAsync(tab.data(), ctx->wb_segs.p, tab.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(seq_seg.data(), seq_seg_dev, seq_seg.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(&total, seq_seg_dev + (size_t)nseq * 2, 4, hipMemcpyDeviceToHost, ctx->stream));
        slot_sync(ctx, ctx->stream);
        int o = 0;
        for (int i = 0; i < nseq; ++i) {
            seg_off[i] = o;
            const int a = seq_seg[2 * i], n = seq_seg[2 * i + 1];
            if (a < 0 || n < 0 || a + n > cap || n > (seqs[2 * i + 1] + 1) / 2) fail(BBOCR_ERR_INTERNAL, "segment table out of range");
            for (int k = 0; k < n; ++k, ++o) { segs[2 * o] = tab[2 * (size_t)(a + k)]; segs[2 * o + 1] = tab[2 * (size_t)(a + k) + 1]; }
        }
        seg_off[nseq] = o;
        if (total != o) fail(BBOCR_ERR_INTERNAL, "the device's segment count disagrees with its table");
    });
}

int bbocr_op_dict_lookup(bbocr_ctx* ctx, const uint16_t* symbols, const int* word_off, int n_words, int n_slots, const uint16_t* q_symbols,
                         const int* q_off, int n_q, int* found, int* longest_probe) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        if (!q_symbols || !q_off || !found || n_q <= 0 || n_words < 0 || n_slots < 0 || q_off[0] != 0) fail(BBOCR_ERR_ARG, "bad dictionary-lookup arguments");
        for (int q = 0; q < n_q; ++q)
            if (q_off[q + 1] < q_off[q] || q_off[q + 1] - q_off[q] > WD_WORD_MAX) fail(BBOCR_ERR_ARG, "a query of more than 1024 symbols, or offsets that descend");
        const int qtotal = q_off[n_q];
        std::vector<unsigned char> qbytes((size_t)std::max(qtotal, 1));
        for (int i = 0; i < qtotal; ++i) {
            if (q_symbols[i] > 255) fail(BBOCR_ERR_ARG, "the device table holds byte symbols");
            qbytes[i] = (unsigned char)q_symbols[i];
        }
        WordDictDev d = ctx->wd_dev;
        WdTable t;
        DevBuf tmp;
        std::vector<unsigned char> stage;
        if (n_words > 0) {
            if (!wd_build(symbols, word_off, n_words, 128, /*space: none*/ -1, (uint32_t)n_slots, t)) fail(BBOCR_ERR_ARG, "bad dictionary or slot count");
            d = upload_dict(t, tmp, stage, ctx->stream);
            if (longest_probe) *longest_probe = t.longest_probe;
        } else {
            if (!d.slots) fail(BBOCR_ERR_ARG, "the context has no dictionary on the device");
            if (longest_probe) *longest_probe = d.probe;
        }
        DevBuf qd;
        const size_t off_bytes = ((size_t)n_q + 1) * 4, found_off = (off_bytes + qbytes.size() + 3) & ~(size_t)3;
        qd.ensure(found_off + (size_t)n_q * 4);
        HIPCHK(hipMemcpyAsync(qd.p, q_off, off_bytes, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync((char*)qd.p + off_bytes, qbytes.data(), qbytes.size(), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(launch_dict_lookup(d, (const unsigned char*)qd.p + off_bytes, (const int*)qd.p, n_q, qtotal, (int*)((char*)qd.p + found_off), ctx->stream));
        std::vector<int> res((size_t)n_q);
        HIPCHK(hipMemcpyAsync(res.data(), (char*)qd.p + found_off, (size_t)n_q * 4, hipMemcpyDeviceToHost, ctx->stream));
        slot_sync(ctx, ctx->stream);
        memcpy(found, res.data(), (size_t)n_q * 4);
    });
}

int bbocr_op_ctc_wordbeam(bbocr_ctx* ctx, const float* dev_probs, size_t rows, const int* seqs, int nseq, int C, int cs, int beam_width, int* text_off,
                          int* text_idx) {
    return guarded(ctx, [&](bbocr_ctx* ctx) {
        if (!dev_probs || !seqs || !text_off || !text_idx || nseq <= 0 || rows > (size_t)INT32_MAX || C <= 0 || C > 128 || cs < C || beam_width < 1 ||
            beam_width > BBOCR_BEAM_DEVICE_MAX)
            fail(BBOCR_ERR_ARG, "bad word-beam-search arguments");
        if (!ctx->wd_dev.slots || !ctx->wd_host) fail(BBOCR_ERR_ARG, "the context has no dictionary (bbocr_set_dictionary)");
        if (ctx->wd_host->space >= C) fail(BBOCR_ERR_ARG, "the dictionary's space class lies outside these rows' classes");
        int max_T;
        check_seqs(seqs, nseq, rows, max_T);
        if (!ctc_wordbeam_on_device(beam_width, C, max_T)) fail(BBOCR_ERR_ARG, "the longest sequence does not fit the device search at this width");
        ctx->seq_tables.ensure((size_t)nseq * 8);
        HIPCHK(hipMemcpyAsync(ctx->seq_tables.p, seqs, (size_t)nseq * 8, hipMemcpyHostToDevice, ctx->stream));
        wordbeam_device(ctx, dev_probs, nullptr, rows, C, cs, seqs, (const int*)ctx->seq_tables.p, nseq, beam_width, ctx->stream);
        std::vector<int> bidx(rows), blen(nseq);
        if (rows) HIPCHK(hipMemcpyAsync(bidx.data(), ctx->ctc_beam_idx.p, rows * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(blen.data(), ctx->ctc_beam_len.p, (size_t)nseq * 4, hipMemcpyDeviceToHost, ctx->stream));
        slot_sync(ctx, ctx->stream);
        int o = 0;
        for (int i = 0; i < nseq; ++i) {
            text_off[i] = o;
            const int n = std::clamp(blen[i], 0, seqs[2 * i + 1]);
            for (int k = 0; k < n; ++k) text_idx[o++] = bidx[(size_t)seqs[2 * i] + k];
        }
        text_off[nseq] = o;
    });
}

}   // extern "C"
