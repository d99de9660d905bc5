// The look-ahead Cholesky sweep of the (mrows x np) column-major lower matrix F (mrows >= np; the rows beyond np are "augmented"
// right-hand-side rows that receive the forward substitution for free): plan, named events, steps, one function per schedule.
// DESIGN.md section 4 has the picture.
#include "ctx.h"

// The leaf level: 128 columns at a time (leaf_potrf -> trsm_rows -> inner update of the rest of the block, K = 128).
// rows_end(nb) = one past the last row that takes part once nb column blocks are factored
struct RowEnd { long eoff; bool winv; long operator()(int nb) const { return winv ? eoff + (long)nb * 128 : eoff; } };

// mark / mark_step: record `mark` on the stream after the mark_step-th kernel of the chain (1 = first leaf, 2 = its trsm,
// 3 = its inner update, ...): the caller holds other work back until the chain has got that far
static int factor_panel(pgp_ctx* c, double* F, long ld, RowEnd re, int s0, int s1, hipStream_t st,
                        double* packs = nullptr, int info_base = 0, hipEvent_t mark = nullptr, int mark_step = 0) {
    if (!packs) packs = c->inv16;
    // the diagonal-panel chain of a look-ahead sweep (mark != null or a scratch factorisation next to bulk work): its kernels
    // mark their CUs so that the bulk workgroups there give way
    const bool chain = c->yield && c->yield_flags && packs == c->dpack;
    unsigned* yfl = chain ? c->yield_flags : nullptr;
    int step = 0;
    auto stepped = [&]() -> int {
        if (mark && ++step == mark_step) HIP_TRY(hipEventRecord(mark, st));
        return PGP_OK;
    };
    if (mark && mark_step <= 0) HIP_TRY(hipEventRecord(mark, st));
    for (int cb = s0; cb < s1; ++cb) {
        double* Acc = F + (long)cb * 128 + (long)cb * 128 * ld;
        double* pack = packs + (long)cb * PACK_DOUBLES;
        {
            ProfScope ps(c, PC_LEAF, 128.0 * 128.0 * 128.0 / 3.0, 0.0, st);
            CHK(leaf_potrf_launch(Acc, ld, pack, c->info_dev, info_base + cb * 128, st, nullptr, yfl, c->leaf_pivot));
        }
        CHK(stepped());
        const long rows_below = re(cb + 1) - (long)(cb + 1) * 128;
        if (rows_below > 0) {
            ProfScope ps(c, PC_TRSM, (double)rows_below * 128.0 * 128.0, 0.0, st);
            CHK(trsm_rows_launch(Acc + 128, ld, rows_below, Acc, ld, pack, st, yfl, c->trsm_lean == 2 || (c->trsm_lean == 1 && chain)));
        }
        CHK(stepped());
        if (cb + 1 < s1) {               // inner update of the rest of this outer panel, K = 128
            GemmArgs g{};
            g.A = Acc + 128; g.lda = ld; g.a_kc = 0;
            g.B = Acc + 128; g.ldb = ld; g.b_kc = 0;
            g.C = F + (long)(cb + 1) * 128 + (long)(cb + 1) * 128 * ld; g.ldc = ld;
            g.M = (int)rows_below; g.N = (s1 - 1 - cb) * 128; g.K = 128;
            g.alpha = -1.0; g.beta = 1.0; g.tri = 1; g.tri_off = 0; g.mask_diag = 1; g.kmode = KM_FULL;
            const long t128 = (long)(g.M / 128) * (g.N / 128);
            g.tile = t128 < c->small_tile_below ? 64 : 128;
            g.flops = 2.0 * 128.0 * ((double)g.M * g.N - 0.5 * (double)g.N * g.N);
            if (chain) g.yield_role = 2;
            CHK(gemm_prof(c, PC_GEMM_INNER, g, st));
        }
        CHK(stepped());
    }
    if (mark && step < mark_step) HIP_TRY(hipEventRecord(mark, st));      // a chain shorter than mark_step
    return PGP_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Cholesky sweep ("diagonal-panel" schedule).
//
// Only the w x w DIAGONAL block of an outer panel (w = 128 q = 512) goes through the leaf-level factorisation, in a small
// scratch with identity rows appended so that E_D = L_D^-T falls out with it (D(p), a chain of 13 small
// launches: stage in | 4 x [leaf_potrf, trsm_rows, K = 128 update] | stage out).  Everything below the block is then ONE MFMA GEMM per panel
//        Y = X E_D        (S(p);  K clipped to the triangle, k < j0 + T)
// and the trailing update TU(p) is one K = w product.  Depth-1 look-ahead on two streams:
//
//   main :  S(p) -> TU_a(p) [next panel's columns, written to the staging buffer Xs] -> TU_b(p) [rest, in place] -> ...
//   panel:                       D(p+1) (reads its diagonal block from Xs)  ..................^ joined before S(p+1)
//
// S is out of place (reads Xs, writes the factor / inverse rows), which is free: TU_a already reads and writes those
// columns once, it just writes them to Xs instead.  The matrix lives in two pieces: logical rows [0, mrows) in F
// (factor + rhs rows, what a posterior handle keeps) and rows [mrows, mrows + np) in E (fused inverse, scratch): with
// the inverse rows riding through the sweep like the augmented right-hand-side rows, E <- E L^-T = L^-T = W^T.  Row i of
// E stays zero left of its own column block, so after nb factored column blocks only the first 128 nb rows of E take part:
// the extra work is N^3/3 flops -- exactly a triangular inverse -- inside the big K = w trailing-update launches.
// dense2 > 0: the second piece is NOT the fused inverse but dense2 extra right-hand-side rows (all of them take part from
// the first panel on: they receive the forward substitution X <- X L^-T, like the rhs rows inside F)
struct SweepMat { double* F; long ldf; long mrows; double* E; long lde; long np; long dense2 = 0;
                  long rows2(int blocks) const { return !E ? 0 : (dense2 > 0 ? dense2 : (long)blocks * 128); } };

static int ensure_stage(pgp_ctx* c, long rows, int w) {
    const size_t need = (size_t)rows * w * sizeof(double);
    if (c->Xs_bytes >= need) return PGP_OK;
    (void)hipStreamSynchronize(c->st);
    if (c->Xs) (void)hipFree(c->Xs);
    c->Xs = nullptr; c->Xs_bytes = 0;
    HIP_TRY(hipMalloc((void**)&c->Xs, need));
    c->Xs_bytes = need;
    return PGP_OK;
}

// D: factor the w x w block `src` (leading dimension lds, lower part) and produce E_D = L_D^-T beside it: L_D -> Fd (ldf),
// E_D -> Ed (lde; may be null), E_D also stays in c->Dk + w (leading dimension 2w) for the panel solve that follows
// Dk: the 2w x w scratch.  In two halves, so that the stage-out can run later and on another stream (s_pan_out)
static int diag_block_factor_in(pgp_ctx* c, const double* src, long lds, int w, int info_base, hipStream_t st, hipEvent_t staged,
                                double* Dk) {
    const long ldd = 2L * w;
    { ProfScope ps(c, PC_DIAG, 0.0, 8.0 * 3.0 * w * w, st);
      CHK(diag_in_launch(src, lds, Dk, ldd, w, st)); }
    return factor_panel(c, Dk, ldd, RowEnd{(long)w, true}, 0, w / 128, st, c->dpack, info_base, staged, c->leaf_first - 1);
}
static int diag_block_out(pgp_ctx* c, int w, double* Fd, long ldf, double* Ed, long lde, hipStream_t st, const double* Dk) {
    ProfScope ps(c, PC_DIAG, 0.0, 8.0 * 3.0 * w * w, st);
    return diag_out_launch(Dk, 2L * w, w, Fd, ldf, Ed, lde, st);
}
int diag_block_factor(pgp_ctx* c, const double* src, long lds, int w, double* Fd, long ldf, double* Ed, long lde,
                      int info_base, hipStream_t st, hipEvent_t staged) {
    CHK(diag_block_factor_in(c, src, lds, w, info_base, st, staged, c->Dk));
    return diag_block_out(c, w, Fd, ldf, Ed, lde, st, c->Dk);
}

// S(p): rows below the diagonal block of panel [s0, s1):  Y = X E_D, X read from the staging buffer (logical rows, ldx)
// (E_D from the scratch Dk; mark: the launch marks its CUs like the chain's own products)
static int solve_below(pgp_ctx* c, const SweepMat& m, int s0, int s1, const double* Xs, long ldx, hipStream_t st,
                       const double* Dk, bool mark) {
    const int w = (s1 - s0) * 128;
    const long r0 = (long)s1 * 128, r1 = m.mrows + m.rows2(s0);
    if (r1 <= r0) return PGP_OK;
    GemmArgs g{};
    g.A = Xs + r0; g.lda = ldx; g.a_kc = 0;
    g.B = Dk + w; g.ldb = 2L * w; g.b_kc = 1;  // B(n,k) = E_D(k,n): K-contiguous
    g.C = m.F + r0 + (long)s0 * 128 * m.ldf; g.ldc = m.ldf;
    if (m.E && r1 > m.mrows) { g.C2 = m.E + (long)s0 * 128 * m.lde; g.ldc2 = m.lde; g.c_split = (int)(m.mrows - r0); }
    g.M = (int)(r1 - r0); g.N = w; g.K = w; g.alpha = 1.0; g.beta = 0.0;
    g.kmode = KM_LT_J; g.koff = 0;
    const long t128 = (long)(g.M / 128) * (w / 128);
    // fewer 128-tiles than workgroup slots: the launch lasts as long as its longest (k = w) tile while the short-k tiles'
    // CUs idle -- 64-tiles, long-k columns first, balance it (option s_tile: 0 = this rule, 64 / 128 = forced)
    g.tile = c->s_tile ? c->s_tile : ((t128 < c->small_tile_below || t128 < 512) ? 64 : 128);
    g.rev_cols = 1;
    const double nt = (double)(w / g.tile);
    g.flops = 2.0 * (double)g.M * g.tile * g.tile * nt * (nt + 1.0) * 0.5;
    if (mark) g.yield_role = 2;
    return gemm_prof(c, PC_GEMM_SOLVE, g, st);
}

// Option skip_zeros: the panel's own inverse rows (rows >= g.zero_from) hold E_D = L_D^-T, upper triangular, so tile row r of them
// starts at k = T r (GemmArgs::zf_upper; T = the tile's rows) instead of multiplying the zeros left of the diagonal -- eet_panel_args
// clips the same structure with KM_GE_I.  g.flops stays what is EXECUTED: the skipped products come off.
static void trailing_skip(pgp_ctx* c, GemmArgs& g) {
    if (!c->skip_zeros || g.zero_from <= 0 || g.zero_from >= g.M) return;
    const int T = g.tile == 64 ? 64 : 128;
    g.zf_upper = 1;
    const double nr = (double)((g.M - g.zero_from) / T);
    g.flops -= (double)T * T * g.N * nr * (nr - 1.0);                // sum_r 2 T N (T r)
}

// TU: columns [c0, c1) -= P P^T, P = solved columns [k0, k1), restricted to the row blocks [rb0, rb1) (rb1 < 0: to the last row that
// takes part); out != nullptr: the result goes to the staging buffer.  rb0 == c0: the rows start at the columns' own diagonal block
// (lower-triangular tile set) -- TU_a, TU_b, and with rb1 == c1 the DIAGONAL BLOCK of the next panel alone, all D(p+1) needs (TU_d);
// rb0 == c1: the rectangle below it (TU_r).  tile 0: by size.
static GemmArgs trailing_update_args(pgp_ctx* c, const SweepMat& m, int k0, int k1, int rb0, int rb1, int c0, int c1,
                                     double* out, long ldx, int tile) {
    const long r0 = (long)rb0 * 128, rend = m.mrows + m.rows2(k1);
    const long r1 = rb1 >= 0 ? (long)rb1 * 128 : rend;
    GemmArgs g{};
    g.A = m.F + r0 + (long)k0 * 128 * m.ldf; g.lda = m.ldf; g.a_kc = 0;
    g.B = m.F + (long)c0 * 128 + (long)k0 * 128 * m.ldf; g.ldb = m.ldf; g.b_kc = 0;
    double* Cf = m.F + r0 + (long)c0 * 128 * m.ldf;
    const bool split = m.E && r1 > m.mrows;
    const int sp = (int)(m.mrows - r0);
    double* Ce = split ? m.E + (long)c0 * 128 * m.lde : nullptr;
    if (split) { g.A2 = m.E + (long)k0 * 128 * m.lde; g.lda2 = m.lde; g.a_split = sp; }
    if (out) {
        g.Cin = Cf; g.ldcin = m.ldf; g.Cin2 = Ce; g.ldcin2 = m.lde;
        g.C = out + r0; g.ldc = ldx;
        if (split) { g.C2 = out + r0 + sp; g.ldc2 = ldx; g.c_split = sp; }
    } else {
        g.C = Cf; g.ldc = m.ldf;
        if (split) { g.C2 = Ce; g.ldc2 = m.lde; g.c_split = sp; }
    }
    g.M = (int)(r1 - r0); g.N = (c1 - c0) * 128; g.K = (k1 - k0) * 128;
    g.alpha = -1.0; g.beta = 1.0; g.kmode = KM_FULL;
    if (rb0 == c0) { g.tri = 1; g.tri_off = 0; g.mask_diag = 1; }
    if (split && !m.dense2) g.zero_from = (int)(m.mrows + (long)k0 * 128 - r0);     // this panel's own inverse rows: first touch
    const long t128 = (long)(g.M / 128) * (g.N / 128) - (long)(g.N / 128) * (g.N / 128 - 1) / 2;
    g.tile = tile ? tile : (t128 < c->small_tile_below ? 64 : 128);
    g.flops = 2.0 * (double)g.K * ((double)g.M * g.N - (rb0 == c0 ? 0.5 * (double)g.N * g.N : 0.0));
    trailing_skip(c, g);
    return g;
}

// Filler: B^-1 (lower) += E_p E_p^T with E_p = columns [s0, s1) of E = L^-T, which are FINAL once S(p) has run (right-
// looking sweep).  E_p is non-zero in rows < 128 s1 only, so the product covers the leading 128 s1 square; its rows
// >= 128 s0 are touched for the first time (zero_from), and inside the diagonal block k starts at the row (KM_GE_I).
static GemmArgs eet_panel_args(pgp_ctx* c, const SweepMat& m, int s0, int s1, double* Binv, long ldb) {
    GemmArgs g{};
    g.A = m.E + (long)s0 * 128 * m.lde; g.lda = m.lde; g.a_kc = 0;
    g.B = g.A; g.ldb = m.lde; g.b_kc = 0;
    g.C = Binv; g.ldc = ldb;
    g.M = s1 * 128; g.N = s1 * 128; g.K = (s1 - s0) * 128; g.alpha = 1.0; g.beta = s0 > 0 ? 1.0 : 0.0;
    g.tri = 2; g.mask_diag = 1; g.kmode = KM_GE_I; g.koff = -s0 * 128;
    if (s0 > 0) g.zero_from = s0 * 128;
    const long t128 = (long)s1 * (s1 + 1) / 2;
    g.tile = (t128 < c->small_tile_below || c->eet_tile == 64) ? 64 : 128;
    const double w = (double)g.K, r0 = 128.0 * s0;
    g.flops = w * r0 * r0 + w * w * r0 + w * w * w / 3.0;      // old x old (lower) + new x old (k >= row) + new x new
    return g;
}
static int eet_panel(pgp_ctx* c, const SweepMat& m, int s0, int s1, double* Binv, long ldb, hipStream_t st) {
    return gemm_prof(c, PC_GEMM_LAUUM, eet_panel_args(c, m, s0, s1, Binv, ldb), st);
}

// ---- the plan: every decision of one sweep, taken once -----------------------------------------------------------------
struct SweepPlan {
    int nblk, q, npanel;     // 128-column blocks, blocks per panel, panels
    long ldx;                // staging buffer, indexed by logical row
    bool la; int sched;      // depth-1 look-ahead on two streams; the effective schedule: 0, 1 or 2
    bool span, span_out, lf; // sched 2: S(p) on the panel stream; D(p)'s stage-out off the chain; leaf_first
    bool fill_inline, fill2; // panel p's share of E E^T / of the caller's C -= R R^T behind TU_b(p)
    int pf, tur_tile;        // fill_inline: panels 0 .. pf go into one product; tile of TU_r
};

static SweepPlan sweep_plan(pgp_ctx* c, const SweepMat& m, const SweepJob& job) {
    SweepPlan pl{};
    const int nblk = pl.nblk = (int)(m.np / 128);
    // panel width: 512 columns; 1024 from N = 12288 on (measured: the K = 1024 updates and the halved number of chain
    // steps win 1.4 % at N = 12288, 1.6 % at 16384, 3 % at 20480; at N = 8192 the 512-wide panels win by 4 %)
    const int q = pl.q = c->nb_outer > 0 ? std::min(c->nb_outer, 8) : (nblk >= 96 ? 8 : 4);
    const int npanel = pl.npanel = (nblk + q - 1) / q;
    pl.ldx = m.mrows + (m.dense2 > 0 ? m.dense2 : m.np);
    const bool la = pl.la = c->lookahead && npanel >= 3;
    // B^-1 = sum_p E_p E_p^T accumulated under the sweep (eet_overlap 2, or 3 up to eet_max_panels panels: beyond that the
    // chain is amortised and the one-shot long-K product is faster): panel p's share right behind TU_b(p) on the main
    // stream -- the main stream stays busy until D(p+1) is done instead of waiting for it
    pl.fill_inline = la && m.E && !m.dense2 && job.eet_out &&
                     (c->eet_overlap == 2 || (c->eet_overlap == 3 && npanel <= c->eet_max_panels));
    // the first products are small (few tiles, short k) and the early trailing updates are long enough to hide D by
    // themselves: panels 0 .. eet_first go into ONE product (k = (eet_first + 1) w) behind TU_b(eet_first)
    pl.pf = std::min(c->eet_first >= 0 ? c->eet_first : npanel / 6, npanel - 2);
    // dense right-hand-side rows R (EP: R L^-T = V' = K sW L^-T): the caller's symmetric C -= V' V'^T is accumulated panel by
    // panel behind TU_b as well -- at N = 4096 the sweep is bound by the chain of diagonal blocks and the main stream would
    // wait for D(p+1) anyway
    pl.fill2 = m.dense2 > 0 && job.rhs_C != nullptr;
    // sched 1 (round 5): the CRITICAL PATH  D(p) -> S(p) -> TU_a(p) -> D(p+1)  lives on the (high-priority) panel stream, the bulk --
    // TU_b(p) + E E'(p) -- on the main stream.  The two under-filled launches of a panel (S: ~250 tile units, TU_a: ~230) then run
    // BESIDE the previous panel's bulk launch and its tail instead of alone on the chip between two bulk launches, and D(p+1) starts
    // without waiting for them to drain a full chip.  Events: main waits for S(p) before TU_b(p); the panel stream waits for
    // TU_b(p-1) (which brought panel p+1's columns up to date) before TU_a(p).  Same launches with the same arguments as sched 0, on other
    // streams: bit-identical to sched 0.  NOT to sched 2, whose TU_d runs the next panel's diagonal block as 64-tiles: those start their
    // accumulators from C, the 128 x 128 LDS-DMA tiles of TU_a fold C in during the k-loop (gemm_tile.h, "lazy C") -- the same sum in
    // another order, a few 1e-13 relative in alpha (tests/test_gpu_side_by_side.py pins both statements).
    // sched 1 is what fit streams that run side by side ask for (_lib.concurrent_fit_streams); it pays from N ~ 7000 on (two streams,
    // N = 8192: 109.5 vs 107.7 fits/s with sched 2) and costs below (N = 6144: 218.5 vs 225.3; N = 4096: 467 vs 513 / 521 with
    // sched 2 / 0): smaller sweeps take the default schedule instead
    const int sched_req = (c->concurrent_streams && !c->sched_explicit) ? 1 : c->sched;     // fit streams side by side: sched 1 unless the user chose
    const int sched_eff = (sched_req == 1 && nblk < 56) ? PGP_SCHED_DEFAULT : sched_req;
    const bool sched1 = la && sched_eff == 1 && !m.dense2;
    // sched 2 pays for 512-wide panels only (N = 4096: -3.6 %, N = 8192: -2.1 %); with 1024-wide panels the diagonal-block piece is
    // 136 K = 1024 tiles and the rectangle it disturbs twice as long: N = 16384 68.9 -> 70.3 ... 71.2 ms -- those keep schedule 0
    // ... and only with the fused inverse rows in the sweep: a plain factorisation (jitchol, EP's post.L) is bound by the chain on a
    // mostly idle chip, where the extra event and the marked piece only add to it (EP's final factor with 512-wide panels: 17.5 ->
    // 18.0 ms per fit with sched 2)
    // ... and from N = 4096 on (measured: N = 2048 1.267 -> 1.313 ms, N = 4096 2.94 -> 2.88, N = 8192 11.13 -> 10.90)
    const bool sched2 = la && sched_eff == 2 && !m.dense2 && m.E != nullptr && ((q <= 4 && nblk >= 32 && nblk < 72) || c->sched2_wide);     // N = 6144: 6.08 -> 5.78 ms; N = 10240: 19.67 -> 19.76
    pl.sched = sched1 ? 1 : (sched2 ? 2 : 0);
    pl.span = sched2 && !c->leaf_first && c->s_pan != 0;
    // the stage-out of D(p) off the chain; the scratch is double-buffered by panel parity (2w x w doubles each, w <= 512: the two
    // halves of c->Dk), so that D(p+1) may stage in while S(p) / the stage-out of D(p) still read D(p)'s
    pl.span_out = pl.span && c->s_pan_out && q <= 4;
    // leaf_first: the trailing update is held back until D(p+1)'s stage-in is done, so that the first leaf is dispatched
    // BEFORE the update's first wave takes every workgroup slot (a leaf dispatched into that wave waits ~140 us for it)
    pl.lf = la && c->leaf_first;
    pl.tur_tile = c->tur_tile ? c->tur_tile : (nblk <= 40 ? 1264 : 128);
    return pl;
}

// ---- the look-ahead hand-off events of one sweep, by meaning -----------------------------------------------------------------
// Index map into c->la_ev, n = npanel; the ranges are disjoint, and this is the one place that sizes the vector:
//   [0, n) s_done | [n, 2n) bulk_done | [2n, 3n) next_cols_staged | [3n, 4n) d_done | [4n, 5n) rows_staged | 5n start | 5n + 1, 5n + 2 leaf_mark
struct SweepEvents {
    const hipEvent_t* ev = nullptr; int n = 0;
    int init(pgp_ctx* c, const SweepPlan& pl) {
        n = pl.npanel;
        if (pl.la) CHK(ensure_events(c->la_ev, 5 * (size_t)n + 3));
        ev = c->la_ev.data();
        return PGP_OK;
    }
    hipEvent_t s_done(int p) const { return ev[p]; }                      // S(p) done; panel -> main (sched 1; s_pan)
    hipEvent_t bulk_done(int p) const { return ev[n + p]; }               // TU_b(p) [+ E E'(p)] queued; main -> panel: TU_a(p+1) / TU_d(p+1) (sched 1; s_pan_direct)
    hipEvent_t next_cols_staged(int p) const { return ev[2 * n + p]; }    // main has staged (or no longer touches) what the panel stream needs of panel
                                                                          // p+1's columns; main -> panel: D(p+1), or TU_d(p) in sched 2 (sched 0 / 2)
    hipEvent_t d_done(int p) const { return ev[3 * n + p]; }              // D(p) done; panel -> main
    hipEvent_t rows_staged(int p) const { return ev[4 * n + p]; }         // TU_a(p)'s rows below the diagonal block are staged; main -> panel: S(p+1) (s_pan)
    hipEvent_t start() const { return ev[5 * n]; }                        // panel 0's staging copy and D(0) ran on main; main -> panel (sched 1)
    hipEvent_t leaf_mark(int parity) const { return ev[5 * n + 1 + parity]; }  // inside D's chain on the panel stream -> main (leaf_first)
};

// ---- one sweep: the steps, defined once, and the schedules that queue them ---------------------------------------------------------
struct Sweep {
    pgp_ctx* c; const SweepMat& m; SweepJob& job; const SweepPlan pl; SweepEvents ev;
    hipStream_t main, pan; double* Xs;

    int s0(int p) const { return p * pl.q; }                                  // panel p = column blocks [s0, s1)
    int s1(int p) const { return std::min(p * pl.q + pl.q, pl.nblk); }
    bool last(int p) const { return s1(p) >= pl.nblk; }
    double* Dk(int p) const { return pl.span_out ? c->Dk + (size_t)(p & 1) * 1024 * 1024 : c->Dk; }

    // D(p) in two halves: stage-in + leaf chain in the scratch Dk(p) (src: the block's updated image -- the factor for panel 0, the staging
    // buffer after that), and the stage-out L_D -> F, E_D -> E, possibly on another stream
    int D_in(int p, hipStream_t st, hipEvent_t staged = nullptr) const {
        return diag_block_factor_in(c, p ? Xs + (long)s0(p) * 128 : m.F, p ? pl.ldx : m.ldf, (s1(p) - s0(p)) * 128, s0(p) * 128, st, staged, Dk(p));
    }
    int D_out(int p, hipStream_t st) const {
        const long o = (long)s0(p) * 128;
        return diag_block_out(c, (s1(p) - s0(p)) * 128, m.F + o * (1 + m.ldf), m.ldf, (m.E && !m.dense2) ? m.E + o * (1 + m.lde) : nullptr, m.lde, st, Dk(p));
    }
    int D(int p, hipStream_t st, hipEvent_t staged = nullptr) const { CHK(D_in(p, st, staged)); return D_out(p, st); }
    int S(int p, hipStream_t st, bool mark = false) const { return solve_below(c, m, s0(p), s1(p), Xs, pl.ldx, st, Dk(p), mark); }
    // TU_a(p): the next panel's columns -> staging; in sched 2 in two pieces: TU_d(p), its diagonal block (64-tiles, marked like the chain's
    // products with tud_mark), and TU_r(p), the rectangle below it
    // (tu: panel p's update of the columns [c0, c1), rows [rb0, rb1))
    GemmArgs tu(int p, int rb0, int rb1, int c0, int c1, double* out, int tile = 0) const {
        return trailing_update_args(c, m, s0(p), s1(p), rb0, rb1, c0, c1, out, pl.ldx, tile);
    }
    int TU_a(int p, hipStream_t st) const { return gemm_prof(c, PC_GEMM_TRAIL, tu(p, s1(p), -1, s1(p), s1(p + 1), Xs), st); }
    int TU_d(int p, hipStream_t st) const {
        GemmArgs g = tu(p, s1(p), s1(p + 1), s1(p), s1(p + 1), Xs, c->tud_tile);
        if (c->tud_mark) g.yield_role = 2;
        return gemm_prof(c, PC_GEMM_TRAIL, g, st);
    }
    int TU_r(int p, hipStream_t st) const { return gemm_prof(c, PC_GEMM_TRAIL, tu(p, s1(p + 1), -1, s1(p), s1(p + 1), Xs, pl.tur_tile), st); }
    // bulk(p) on the main stream, concurrent with D(p+1): TU_b(p), the rest of the trailing update in place, and -- fill_inline -- panel
    // p's share of E E'; the two are independent: ONE launch, one tail, where the kernel family allows it (pair_launch)
    int bulk(int p) const {
        const int n1 = s1(p + 1);
        const bool fill_now = pl.fill_inline && p >= pl.pf;
        if (fill_now && n1 < pl.nblk && c->pair_launch)
            return gemm_prof_pair(c, PC_GEMM_TRAIL, tu(p, n1, -1, n1, pl.nblk, nullptr), PC_GEMM_LAUUM,
                                  eet_panel_args(c, m, p == pl.pf ? 0 : s0(p), s1(p), job.eet_out, job.eet_ld), main);
        if (n1 < pl.nblk) CHK(gemm_prof(c, PC_GEMM_TRAIL, tu(p, n1, -1, n1, pl.nblk, nullptr), main));
        if (fill_now) CHK(eet_panel(c, m, p == pl.pf ? 0 : s0(p), s1(p), job.eet_out, job.eet_ld, main));
        return PGP_OK;
    }
    // fill2: the caller's C -= R_p R_p^T, R_p = the solved columns of panel p of the dense right-hand-side rows
    int rhs_product(int p) const {
        GemmArgs g{};
        g.A = m.E + (long)s0(p) * 128 * m.lde; g.lda = m.lde; g.a_kc = 0;
        g.B = g.A; g.ldb = m.lde; g.b_kc = 0;
        g.C = job.rhs_C; g.ldc = job.rhs_ld; g.M = (int)m.dense2; g.N = (int)m.dense2; g.K = (s1(p) - s0(p)) * 128;
        g.alpha = -1.0; g.beta = 1.0; g.tile = 128; g.tri = 2; g.mask_diag = 1;
        g.flops = (double)m.dense2 * m.dense2 * g.K;
        return gemm_prof(c, PC_GEMM_INNER, g, main);
    }

    // common head: panel 0's columns go to the staging buffer by a plain copy (later panels get there through TU_a); D(0) on main
    int head() const {
        const long r0 = (long)s1(0) * 128;
        if (m.mrows > r0)
            HIP_TRY(hipMemcpy2DAsync(Xs + r0, pl.ldx * sizeof(double), m.F + r0, m.ldf * sizeof(double),
                                     (m.mrows - r0) * sizeof(double), (size_t)s1(0) * 128, hipMemcpyDeviceToDevice, main));
        if (m.E && m.dense2 > 0)                                  // the dense second piece takes part from panel 0 on
            HIP_TRY(hipMemcpy2DAsync(Xs + m.mrows, pl.ldx * sizeof(double), m.E, m.lde * sizeof(double),
                                     m.dense2 * sizeof(double), (size_t)s1(0) * 128, hipMemcpyDeviceToDevice, main));
        return D(0, main);
    }

    //   panel:  S(p) -> TU_a(p) -> D(p+1) -> S(p+1) ...          main:  bulk(p) after S(p) ...
    int run_sched1() const {
        HIP_TRY(hipEventRecord(ev.start(), main));
        HIP_TRY(hipStreamWaitEvent(pan, ev.start(), 0));
        for (int p = 0; p < pl.npanel; ++p) {
            CHK(S(p, pan));
            HIP_TRY(hipEventRecord(ev.s_done(p), pan));
            HIP_TRY(hipStreamWaitEvent(main, ev.s_done(p), 0));
            if (last(p)) break;
            if (p >= 1) HIP_TRY(hipStreamWaitEvent(pan, ev.bulk_done(p - 1), 0));
            CHK(TU_a(p, pan));
            CHK(D(p + 1, pan));
            CHK(bulk(p));
            HIP_TRY(hipEventRecord(ev.bulk_done(p), main));
        }
        return PGP_OK;
    }

    // sched 0: the picture above (without look-ahead the panel stream IS the main stream); sched 2: TU_a(p) = TU_d(p) on the panel stream
    // ahead of D(p+1) + TU_r(p) on main; s_pan: S(p), p >= 1, on the panel stream behind D(p)
    int run_sched02() const {
        for (int p = 0; p < pl.npanel; ++p) {
            // s_pan_out: D(p)'s stage-out (L_D -> F, E_D -> E; S(p) reads E_D from the scratch) is off the chain: it runs on the main stream
            // (which has waited for D(p)'s leaf chain) beside S(p), ahead of TU_r(p) -- the first reader of E_D's copy in E
            if (pl.span_out && p >= 1) CHK(D_out(p, main));
            if (pl.span && p >= 1) {
                // s_pan: S(p) does not wait for the END of the paired launch of panel p - 1 (which D(p) beats by ~35 us): it follows
                // D(p) on the panel stream and runs in that launch's tail.  It reads the staging rows TU_r(p-1) wrote (main stream)
                HIP_TRY(hipStreamWaitEvent(pan, ev.rows_staged(p - 1), 0));
                CHK(S(p, pan, c->s_pan == 2));
                HIP_TRY(hipEventRecord(ev.s_done(p), pan));
                HIP_TRY(hipStreamWaitEvent(main, ev.s_done(p), 0));
            } else {
                CHK(S(p, main));
            }
            if (pl.fill2 && last(p)) CHK(rhs_product(p));
            if (last(p)) break;
            const long rows_end = m.mrows + m.rows2(s1(p));
            if (pl.sched == 2 && rows_end > (long)s1(p + 1) * 128) {
                // sched 2: D(p+1) needs the next panel's DIAGONAL BLOCK only -- that piece of TU_a (64-tiles: a K = w 128-tile alone
                // on a CU lasts as long as the whole of TU_a) goes to the panel stream right behind S(p), the rectangle below it
                // stays on the main stream: D(p+1) starts ~50 us earlier, and its first kernels find free slots beside the
                // one-workgroup-per-CU rectangle instead of the first wave of the bulk launch
                if (pl.span && p >= 1 && c->s_pan_direct) {
                    // S(p) sits on the panel stream already: the piece only needs the paired launch of panel p - 1 (its event), not a
                    // round trip through the main stream's wait for S(p) (26 us between S(p) and the piece before)
                    HIP_TRY(hipStreamWaitEvent(pan, ev.bulk_done(p - 1), 0));
                } else {
                    HIP_TRY(hipEventRecord(ev.next_cols_staged(p), main));
                    HIP_TRY(hipStreamWaitEvent(pan, ev.next_cols_staged(p), 0));
                }
                CHK(TU_d(p, pan));
                CHK(TU_r(p, main));
            } else {
                CHK(TU_a(p, main));
                if (pl.la) {
                    HIP_TRY(hipEventRecord(ev.next_cols_staged(p), main));
                    HIP_TRY(hipStreamWaitEvent(pan, ev.next_cols_staged(p), 0));
                }
            }
            if (pl.span) HIP_TRY(hipEventRecord(ev.rows_staged(p), main));
            if (pl.span_out) CHK(D_in(p + 1, pan));
            else CHK(D(p + 1, pan, pl.lf ? ev.leaf_mark(p & 1) : nullptr));
            if (pl.lf) HIP_TRY(hipStreamWaitEvent(main, ev.leaf_mark(p & 1), 0));
            if (pl.la) HIP_TRY(hipEventRecord(ev.d_done(p + 1), pan));
            CHK(bulk(p));
            if (pl.fill2) CHK(rhs_product(p));
            if (pl.span) HIP_TRY(hipEventRecord(ev.bulk_done(p), main));        // what TU_d(p+1) waits for
            if (pl.la) HIP_TRY(hipStreamWaitEvent(main, ev.d_done(p + 1), 0));
        }
        return PGP_OK;
    }

    // common tail (fill_inline): the last product has nothing of the sweep left to hide: it goes to the (now idle) panel stream so that the
    // O(N^2) kernels that follow the sweep on the main stream (alpha = E z, log det) run beside it; the caller joins on job.join
    int tail() const {
        if (!pl.fill_inline) return PGP_OK;
        CHK(ensure_events(c->fill_ev, 2));
        HIP_TRY(hipEventRecord(c->fill_ev[0], main));
        HIP_TRY(hipStreamWaitEvent(pan, c->fill_ev[0], 0));
        CHK(eet_panel(c, m, s0(pl.npanel - 1), pl.nblk, job.eet_out, job.eet_ld, pan));
        HIP_TRY(hipEventRecord(c->fill_ev[1], pan));
        job.join = c->fill_ev[1];
        return PGP_OK;
    }
};

// Entry point.  job.inverse: the np rows [mrows, mrows + np) end up holding E = L^-T (upper triangular); the sweep writes EVERY entry
// of the inverse rows it later reads.  job.R: a second piece of nrhs2 dense right-hand-side rows instead (row n, column k at
// R[n + k ldr]): on return row n of R holds (L^-1 r_n)'; the rows ride along in the panel solves and trailing updates of the sweep
// (N^2 flops per row inside the bulk MFMA launches).
int potrf_blocked(pgp_ctx* c, SweepJob& job) {
    job.join = nullptr;
    SweepMat m{job.F, job.ldf, job.mrows, nullptr, 0, job.np};
    // two-piece row space: the panel solves / updates address "rows >= mrows" through a split that must be positive for
    // every panel, i.e. at least one spare row block between the factor's rows and the second piece
    if (job.R || job.nrhs2) {
        if (!job.R || job.nrhs2 <= 0 || job.nrhs2 % 128 || job.mrows < job.np + 128) return -1;
        m.E = job.R; m.lde = job.ldr; m.dense2 = job.nrhs2;
    } else if (job.inverse) {
        m.E = job.E ? job.E : job.F + job.mrows; m.lde = job.E ? job.lde : job.ldf;
        if (m.E != job.F + job.mrows && job.mrows < job.np + 128) return -1;
    }
    Sweep s{c, m, job, sweep_plan(c, m, job), {}, c->st, nullptr, nullptr};
    s.pan = s.pl.la ? c->st2 : c->st;
    CHK(ensure_stage(c, s.pl.ldx, s.pl.q * 128));
    s.Xs = c->Xs;
    CHK(s.ev.init(c, s.pl));
    CHK(s.head());
    CHK(s.pl.sched == 1 ? s.run_sched1() : s.run_sched02());
    return s.tail();
}
