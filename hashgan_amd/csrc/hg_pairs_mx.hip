// libhashgan_amd.so -- launchers of the matrix-core pair passes and of the images they read: k_select_mx3 / mx4
// (optimistic record pass), k_hist_mx / k_hist_i8 (histograms).
#include "hg_ctx.hpp"
#include "hg_mx_drain.hpp"
#include "hg_select_mx.hpp"
#include "hg_select_mx3.hpp"
#include "hg_select_mx4.hpp"
#include "hg_hist_mx.hpp"
#include "hg_hist_i8.hpp"

// the fp4 images of the codes in MFMA fragment order (k_select_mx, k_hist_mx; k_select_mx3 / mx4 share the query image), built on
// first use.  need_db = false: the query image only (k_select_mx3 / mx4 have their own database images)
int ensure_mx_images(hg_ctx* c, const bool need_db) {
    const int NW = c->NW, NM = (NW + 1) / 2;
    if (need_db && !c->dbx_valid) {
        const i64 n16 = (c->N + 15) / 16 * 16;
        HG_TRY(c->dbx.reserve((size_t)(n16 > 0 ? n16 : 16) * NM * 32));
        const i64 items = n16 * 2 * NM;
        c->t_begin(KI_PACK);
        if (items) hipLaunchKernelGGL(k_expand_db, dim3(grid_for(items)), dim3(256), 0, c->stream, c->db.as<u32>(),
                                      c->dbx.as<uint4>(), (i64)c->N, n16, NW, NM);
        c->t_end();
        HG_TRY(c->check_launch("k_expand_db"));
        c->dbx_valid = true;
    }
    if (!c->qx_valid) {
        const i64 qpad = ((i64)c->Q + 511) / 512 * 512;
        HG_TRY(c->qx.reserve((size_t)qpad * NM * 32));
        const i64 items = qpad * 2 * NM;
        c->t_begin(KI_PACK);
        hipLaunchKernelGGL(k_expand_queries, dim3(grid_for(items)), dim3(256), 0, c->stream, c->qc.as<u32>(), c->qx.as<uint4>(),
                           (i64)c->Q, qpad, NW, NM);
        c->t_end();
        HG_TRY(c->check_launch("k_expand_queries"));
        c->qx_valid = true;
    }
    return HG_OK;
}


namespace {
template <int NW> int launch_hist_mx_t(hg_ctx* c) {
    HG_TRY(ensure_mx_images(c, true));
    Geo g = c->geo;                                    // fine geometry; the kernel pairs the segments itself
    const int nSP = (g.S + 1) / 2;
    const int nQB = (g.Q + 255) / 256;
    g.nQT = nQB;
    g.nUnits = (i64)nSP * nQB;
    g.wpb = WPB;
    g.nBlk = (int)g.nUnits;
    const i64 tiles_per_half = ((g.L + 15) / 16 + g.hist_stride - 1) / g.hist_stride;      // visited by one lane-half
    const i64 visited_per_pair = 2 * tiles_per_half * 16;
    const bool pack16 = visited_per_pair < 65536;
    const size_t lds = (size_t)WPB * (pack16 ? 1 : 2) * g.NB * 32 * 4;
    c->last_hist = pack16 ? 2 : 6;
    c->t_begin(KI_HIST);
    if (pack16) {
        hipLaunchKernelGGL((k_hist_mx<NW, true>), dim3(padded_grid(g.nBlk)), dim3(256), lds, c->stream, c->qc.as<u32>(), c->qx.as<u8>(),
                           c->dbx.as<u8>(), c->hist.as<u32>(), g);
    } else {
        if (lds > 64 * 1024)
            HG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_hist_mx<NW, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_hist_mx<NW, false>), dim3(padded_grid(g.nBlk)), dim3(256), lds, c->stream, c->qc.as<u32>(), c->qx.as<u8>(),
                           c->dbx.as<u8>(), c->hist.as<u32>(), g);
    }
    c->t_end();
    return c->check_launch("k_hist_mx");
}

// The packed record pass of the optimistic step (k_select_mx3 / k_select_mx4, one-byte records through the batched drain of
// hg_packed_drain.hpp); blocks = (pair of segments) x (512 queries); the query image is k_select_mx's.  P = the packing's
// traits; `image` is its database image (P::IMG_WORDS code words of 16 bytes per row), built here on first use.
template <class P, class Expand, class Kernel>
int launch_select_packed(hg_ctx* c, const int* cut, const int NW, const int LW, DevBuf& image, bool& image_valid, Expand expand,
                         const char* expand_name, Kernel kernel, const char* kernel_name) {
    HG_TRY(ensure_mx_images(c, false));
    if (!image_valid) {
        const i64 n = (c->N + P::ROWS - 1) / P::ROWS * P::ROWS + P::WS_MAX * P::ROWS;     // + one window of zero rows: the last segment's last window may run past the end
        HG_TRY(image.reserve((size_t)n * P::IMG_WORDS * 16));
        const i64 items = n * P::IMG_WORDS;
        c->t_begin(KI_PACK);
        hipLaunchKernelGGL(expand, dim3(grid_for(items)), dim3(256), 0, c->stream, c->db.as<u32>(), image.as<uint4>(), (i64)c->N, n, NW);
        c->t_end();
        HG_TRY(c->check_launch(expand_name));
        image_valid = true;
    }
    Geo g = c->geo;
    const int nSP = (g.S + 1) / 2;
    const int nQB = (g.Q + 64 * P::WPB - 1) / (64 * P::WPB);
    g.nQT = nQB;
    g.nUnits = (i64)nSP * nQB;
    g.wpb = P::WPB;
    g.nBlk = (int)g.nUnits;
    const PackedLds L = packed_lds_layout<P>(NW, LW);
    if (L.total > 64 * 1024)
        HG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, L.total));
    SelArgs a{cut, c->sl_start.as<u32>(), c->sl_tie.as<u32>(), c->sl_cnt.as<u32>(),
              c->failq.as<u32>(), c->cap, c->crow, 1, c->sstar.as<int>(), (int)c->opt.probe_select};
    c->t_begin(KI_SELECT_MX);
    hipLaunchKernelGGL(kernel, dim3(padded_grid(g.nBlk)), dim3(64 * P::WPB), (size_t)L.total, c->stream, c->qc.as<u32>(),
                       c->qlab.as<u64>(), c->qx.as<u8>(), c->db.as<u32>(), image.as<u8>(), c->dblab.as<u64>(), a,
                       c->cand.as<u8>(), g);
    c->t_end();
    return c->check_launch(kernel_name);
}
template <int NW, int LW> int launch_select_mx3_t(hg_ctx* c, const int* cut) {      // codes of <= 64 bits: three rows per accumulator
    return launch_select_packed<M3Pack>(c, cut, NW, LW, c->dbx3, c->dbx3_valid, k_expand_db3, "k_expand_db3", &k_select_mx3<NW, LW>, "k_select_mx3");
}
template <int NW, int LW> int launch_select_mx4_t(hg_ctx* c, const int* cut) {      // codes of 65..128 bits: two rows per accumulator
    return launch_select_packed<M4Pack>(c, cut, NW, LW, c->dbx4, c->dbx4_valid, k_expand_db4, "k_expand_db4", &k_select_mx4<NW, LW>, "k_select_mx4");
}

// the same pass with the integer matrix instruction delivering the counter addresses (hg_hist_i8.hpp); codes of <= 128 bits
template <int NW> int launch_hist_i8_t(hg_ctx* c, u64* tot) {
    if (!c->dbx8_valid) {
        const i64 n16 = (c->N + 15) / 16 * 16;
        HG_TRY(c->dbx8.reserve((size_t)n16 * NW * 32));
        c->t_begin(KI_PACK);
        hipLaunchKernelGGL(k_expand_db_i8, dim3(grid_for(n16 * NW * 2)), dim3(256), 0, c->stream, c->db.as<u32>(), c->dbx8.as<uint4>(),
                           (i64)c->N, n16, NW);
        c->t_end();
        HG_TRY(c->check_launch("k_expand_db_i8"));
        c->dbx8_valid = true;
    }
    Geo g = c->geo;
    const int nSP = (g.S + 1) / 2;
    const int nQB = (g.Q + 255) / 256;
    g.nQT = nQB;
    g.nUnits = (i64)nSP * nQB;
    g.wpb = WPB;
    g.nBlk = (int)g.nUnits;
    const i64 tiles_per_half = ((g.L + 15) / 16 + g.hist_stride - 1) / g.hist_stride;
    const bool pack16 = 2 * tiles_per_half * 16 < 65536;
    const size_t lds = (size_t)WPB * hist_i8_cols(pack16) * g.NB * 32 * 4;
    c->last_hist = pack16 ? 3 : 7;
    c->t_begin(KI_HIST);
    if (pack16) {
        if (lds > 64 * 1024)
            HG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_hist_i8<NW, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_hist_i8<NW, true>), dim3(padded_grid(g.nBlk)), dim3(256), lds, c->stream, c->qc.as<u32>(), c->dbx8.as<u8>(),
                           c->hist.as<u32>(), tot, g);
    } else {
        if (lds > 64 * 1024)
            HG_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_hist_i8<NW, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_hist_i8<NW, false>), dim3(padded_grid(g.nBlk)), dim3(256), lds, c->stream, c->qc.as<u32>(), c->dbx8.as<u8>(),
                           c->hist.as<u32>(), tot, g);
    }
    c->t_end();
    return c->check_launch("k_hist_i8");
}
}  // namespace

bool hist_i8_applies(const hg_ctx* c) { return c->opt.hist_mfma == 2 && c->NW <= 4; }

int launch_hist_mx(hg_ctx* c, u64* tot) {              // tot: k_hist_i8 also sums its planes over the segment pairs into this table (else nullptr)
    if (hist_i8_applies(c)) {
        switch (c->NW) {
            case 1: return launch_hist_i8_t<1>(c, tot);
            case 2: return launch_hist_i8_t<2>(c, tot);
            case 3: return launch_hist_i8_t<3>(c, tot);
            default: return launch_hist_i8_t<4>(c, tot);
        }
    }
    if (tot) return fail(HG_ERR_STATE, "launch_hist_mx: plane totals come from k_hist_i8 only");
    HG_DISPATCH_NW(launch_hist_mx_t, c)
}


int launch_select_mx4(hg_ctx* c, int lw, const int* cut) {           // codes of 65..128 bits, one-byte records, <= 128 classes
    if (c->NW < 3 || c->NW > 4 || lw < 1 || lw > 2) return fail(HG_ERR_ARG, "k_select_mx4 takes codes of 65..128 bits and 1..128 classes");
    if (c->NW == 3) return lw == 1 ? launch_select_mx4_t<3, 1>(c, cut) : launch_select_mx4_t<3, 2>(c, cut);
    return lw == 1 ? launch_select_mx4_t<4, 1>(c, cut) : launch_select_mx4_t<4, 2>(c, cut);
}

int launch_select_mx3(hg_ctx* c, int lw, const int* cut) {           // codes of <= 64 bits, one-byte records, <= 128 classes
    if (c->NW > 2 || lw < 1 || lw > 2) return fail(HG_ERR_ARG, "k_select_mx3 takes codes of <= 64 bits and 1..128 classes");
    if (c->NW == 1) return lw == 1 ? launch_select_mx3_t<1, 1>(c, cut) : launch_select_mx3_t<1, 2>(c, cut);
    return lw == 1 ? launch_select_mx3_t<2, 1>(c, cut) : launch_select_mx3_t<2, 2>(c, cut);
}

// hg_preload: the runtime loads a translation unit's code object when one of its kernels is first needed (milliseconds);
// asking for a kernel's attributes does that now
int preload_mx() {
    hipFuncAttributes a;
    HG_HIP(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_select_mx3<2, 1>)));
    return HG_OK;
}
