// 3x3 / stride-2 / pad-1 convolution with the input patch resident in LDS as four PARITY PLANES (gfx950): the stride-2 convs of
// the path — BasicBlock conv1 of layers 2-4 and every exit-head conv, SA/models/resnet18/resnet18.py:280-299, :306-329 — on
// conv3x3_pw's 256 x 256 tile / 8 waves / ping-pong main loop, persistent like conv_igemm_wide_persist.
//
// Why.  conv_igemm_wide streams a [256 px][64 ch] activation tile per (tap, 64-channel chunk) from L2: every input line is
// requested 2.25 times per channel tile, and the re-reads miss the XCD's 4 MB L2 (32 workgroups x a 256-px tile's input, with
// the taps of one line 2-8 K-steps apart): rocprofv3 FETCH_SIZE 1.5x (64 -> 128 on 32x32 maps) to 4.2x (256 -> 512 + 512 on 8x8
// maps) the algorithmic input bytes, the kernel at 845 / 985 / 1070 TFLOP/s on the three shape classes against 1270-1420 for
// conv3x3_pw (profiles/experiments/r3_per_launch_before_s2.log).  Here a tile's input is DMA'd ONCE per 32-channel chunk and all
// nine taps are served from LDS.
//
// A stride-2 tap (ky, kx) reads input rows 2 oy + ky - 1 and columns 2 ox + kx - 1: rows of ONE parity per ky, columns of one
// parity per kx.  The patch is therefore kept as four planes — A (odd rows, odd columns; taps (0,0) (0,2) (2,0) (2,2)),
// B (odd, even; (0,1) (2,1)), C (even, odd; (1,0) (1,2)), D (even, even; (1,1)) — inside which a tap is a shift by 0 or 1 cell,
// exactly the stride-1 addressing of conv3x3_pw.  The taps run plane by plane (A A A A B B C C D per 32-channel chunk), so a
// plane's cells are dead long before they are needed again: ONE copy of the patch (72-88 KB for 32 channels) is enough, each
// plane is refilled with the next chunk's channels while the other planes compute (A during the C / D taps, B at the end of
// the period, C and D at the start of their own period), and nothing ever waits for a whole-patch refill.
//
//   tile       = IMGS whole output maps (256 pixels: 1 map of 16x16, 4 of 8x8, 16 of 4x4) x 256 output channels
//   waves      = 2 channel halves (g) x [2 (channels) x 2 (pixels)], wave tile 64 ch x 128 px = 4 x 8 tiles of v_mfma_f32_16x16x32;
//                the 16 pixels of an MFMA tile are a 4 x 4 block of output pixels (conv3x3_pw's tile-pixel order)
//   LDS        = [W0 | W1 | patch pieces | (pad) | last stage] + BN table: three weight stages [256 ch][32 k] (64-byte rows), the patch as
//                NPT pieces of 128 cells x 64 B (piece = one DMA instruction per thread), planes back to back with plane A
//                padded to whole pieces.  132-152 KB: one 512-thread workgroup per CU.
//   64-B rows  = four rows share a 256-byte bank window.  ds_read_b128 is served in four lane groups {0-3, 12-15, 20-27},
//                {4-11, 16-19, 28-31}, ... (MI355X_MICROARCH.md, LDS): a group reads 16-byte chunk kq of rows 0-3 and 12-15 of
//                a 16-row fragment and chunk kq ^ 1 of rows 4-11.  Chunk c of weight row r is stored at position
//                c ^ 2 ((r >> 2) & 1), chunk c of a patch cell in plane row y at c ^ 2 (y & 1): the 16 lanes of every group then
//                hit 16 distinct 16-byte slots, for every tap shift and every cell pitch (tight pitches: TW or TW + 1 cells).
//                LDS-DMA writes lane-linearly, so the permutation is applied to the per-lane SOURCE address.
//   main loop  = conv3x3_pw's: K-step = one tap x 32 channels, two phases (LOAD part / barrier / MFMA part / barrier), the two
//                wave groups one barrier apart, weights of the step AFTER NEXT in flight, counted vmcnt with compile-time
//                immediates (the 9 steps of a chunk are unrolled).  Per step at most two patch pieces ride along.
//   persistent = one workgroup per CU walks the tiles; the next tile's weight stages 0 / 1 and its plane A / B pieces are
//                issued when the main loop ends and land while the epilogue runs (BN + ReLU on the accumulators, fp16 straight from the
//                registers).
//   pair mode  = as conv_igemm_wide: channel tiles >= split use the second conv's weights / BN / output tensor.
//   epilogue   = plain (BN + ReLU) only: every stride-2 conv of the path.  Anything else stays with conv_igemm_wide.
//
// The pad-skip form of the 8x8 -> 4x4 class ("s2_pad_skip" = 1, the default; conv3x3_s2_skip_kernel = the body with SKIP = true; TW == 4, 256-channel
// tiles, fp16 / bf16, single and pair launches, direct and pooled epilogue; row-table launches keep the 4 x 4 blocks).  Output row 0 with ky = 0 and
// output column 0 with kx = 0 read only padding: 23 of the 16 x 9 (position, tap) pairs (16.0 %).  With a 4 x 4 block of ONE image as the MFMA pixel
// tile every tile has a live pixel for every tap.  Here:
//   tile order = conv3x3_pw's pad-skip order (PwGeomSkip): tile pixel p = 128 wp + 16 j + image, pixel tile j of pixel wave wp is the output position
//                (oy, ox) = (j >> 1, 2 (j & 1) + ((oy + wp) & 1)).  Step S (tap (ky, kx) = s2_tap(S)) of a tile is dead exactly when (ky == 0 && oy == 0)
//                || (kx == 0 && ox == 0): a ds_read_b128 and four MFMAs that are not emitted.  Live tiles per wave: tap (0,0) 5 / 4, taps (0,1) (0,2)
//                (1,0) (2,0) 6 / 6, the other four 8 / 8 — the slower wave runs 61 tile-steps per chunk instead of 72 (−15.3 %), 121 of 144 pairs are
//                live (static_asserts below S2Skip).  A step's live tiles go to its two phases in tile order (4 + 4, 3 + 3, 3 + 2, 2 + 2).  Which tiles
//                are dead depends on wp: the chunk loop exists once per pixel wave behind a wave-uniform branch, the same barriers on both sides.  The
//                live sets enter the step as constexpr bit masks: as calls on the unrolled tile index they outlived the inliner in two of the
//                eighteen step bodies — real calls, around MFMAs that ignore EXEC.
//   LDS        = S2Geom untouched: plane sizes, cell0, A_PAD, NPT, pstep, wait_n, the weight stages and everything schedule_ok() checks.  Only the
//                numbering of the cells INSIDE a plane changes: local cell (y * cols(pl) + x) * 16 + img, the image fastest, instead of
//                (img * rows + y) * cols + x — a pixel fragment (16 images of one cell) is 1 KB contiguous.  The padding cells (plane row 0 of the
//                odd-row planes, column 0 of the odd-column planes) keep their slots, their DMA lanes still read beyond the descriptor, and no live
//                tile reads them (S2Skip::cells_ok).  Chunk c of image n sits at position c ^ 2 ((n >> 3) & 1) (conv3x3_pw's): a ds_read_b128 lane
//                group reads images 0-3 and 12-15 at chunk kq and images 4-11 at kq ^ 1, 16 distinct 16-byte slots.  A tap shift and a tile's position
//                are whole cells: compile-time multiples of 1 KB (at most 24 KB) on ONE per-lane offset per plane, boff[pl] (P_OFF + a plane offset does
//                not fit the 16-bit immediate of ds_read).  The images of a ragged last tile lie beyond the per-tile buffer descriptor, as before.
//   K order    = unchanged — chunk-major, steps A A A A B B C C D, 32 channels per MFMA; a product with an all-zero pixel fragment leaves an fp32
//                accumulator as it was, so every output keeps its bits (tests/test_s2_pad_skip.py).
//   epilogues  = direct stores: lane (l16, kq) of tile j is image n0 + l16 at (oy, ox), predicated on n < N.  Pooled: an image's 16 positions are 8
//                tile registers in each of the two pixel waves; they are summed through the staging area at E_OFF in the order of the DPP tree of the
//                4 x 4-block form — per map row (p0 + p1) + (p2 + p3), then (r0 + r1) + (r2 + r3), then * 1/16 (conv3x3_pw's persistent pooled tail):
//                the fp32 results are bit-equal.
//   hazards    = 1. tile-start wait: a wave may leave in flight only the stores it issued BEHIND the next tile's prefetch DMAs.  Per WAVE (vmcnt counts
//                   instructions, whatever the EXEC mask): direct 16, pooled 4 in pixel wave 0 (2 halves x 2 float4) and none in pixel wave 1 — so
//                   vmcnt(16) / vmcnt(4) / vmcnt(0); a ragged tile (lanes beyond N skip their stores: a branch may skip the instruction) drains with
//                   vmcnt(0) as before.
//                2. s_barrier is workgroup-wide: the pooled exchange takes three barriers per 32-channel half = six per tile; in a mixed pair tile the
//                   channel group that stores plainly executes six barriers behind its stores.
//                3. the exchange area (E_OFF .. + 64 KB: the own-period pieces, padding, the last weight stage) is written by the next tile from its
//                   step 0 on (SETUP_TILE issues stages 0 / 1 and the A / B pieces only): the pooled tail ends with lgkmcnt(0), before the tile-start
//                   barrier.
//                4. registers: two step bodies per step.  242 VGPRs, no scratch, no VGPR spill, LDS as the 4 x 4-block form (tools/kernel_resources.py,
//                   tests/test_build_resources.py); the per-lane values (boff[], a_off) do not depend on wp, so nothing was hoisted across the branch.
#include <cstdlib>

#include "conv_epilogue.h"
#include "kernels.h"

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

// The MFMA rows of a wave's four channel tiles are a permutation of its 64 channels (conv3x3_pwp's: row r of tile i = channel
// 32 (i >> 1) + 8 (r >> 2) + 4 (i & 1) + (r & 3)), so a lane holds two runs of 8 consecutive channels per pixel and the epilogue stores them
// straight from the registers — no trip through LDS, no barrier.
// Output stores that bypass the XCD's L2 (sc1, an inline-asm store hipcc does not model) cut rocprofv3 FETCH_SIZE by 12 % at unchanged wall time and were not kept
// (profiles/experiments/r3_s2_sc1_stores.log).

// TW = OUTPUT map size (TW x TW; the input map is 2 TW x 2 TW): 16, 8 or 4.
// NST = 3 weight stages: the weights of K-step T + NST - 1 are issued in step T.  vmcnt retires in order, so waiting for the NEXT
// step's weights also waits for every patch piece issued before them: a piece issued in step s must have landed by the end of
// step s + NST - 1 whether its plane is needed by then or not: 2 K-steps (~1.4 us) for an HBM round trip.  A fourth stage (one more
// K-step) measured 1-2 % slower on all three classes (profiles/experiments/r3_s2_stages_phase.log): the window is not what they wait for.
// MSK = masked input (ConvArgs::in_bits): the patch is DMA'd from the deterministic (pre-scaled) tensor, a piece's keep bits ride
// along as one more DMA (a dword per lane into a 2 KB slot), and the thread that issued a piece clears the dropped elements of
// ITS 16 bytes in LDS one K-step after the piece has landed — a piece is readable one step later than without the mask.
// CT_ = channels per tile: 256, or 128 (round 4, 16x16 output maps only: ResNet-50's Cout = 128 stride-2 convs).  With 128 the two wave groups
// split the tile's PIXELS (output rows 0-7 / 8-15) instead of its channels: a wave tile is 64 ch x 64 px (4 x 4 MFMA tiles), both groups read the
// same 8 KB weight stage, a K-step's two phases take two pixel blocks each (8 MFMAs per phase instead of 16; the barrier schedule, the patch and
// its refill windows are the same).
template <int TW, bool MSK_ = false, int CT_ = 256>
struct S2Geom {
    static_assert(CT_ == 256 || (CT_ == 128 && TW == 16), "128-channel tiles: the 16x16 output maps");
    static constexpr int NST = 3;
    static constexpr bool MSK = MSK_;
    static constexpr int LAND = NST + (MSK ? 1 : 0);              // a piece issued in step s is readable from step s + LAND on
    static constexpr int BN_MAX = TW == 4 ? 1024 : 512;           // channels of the launch (both convs of a pair): the BN table
    static constexpr int CT = CT_, PX = 256, IMGS = PX / (TW * TW);
    static constexpr int WPI = CT / 128;                          // weight DMA instructions per thread and K-step
    static_assert(IMGS >= 1 && IMGS * TW * TW == PX, "whole output maps per tile");
    // planes in tap-use order: 0 = A (odd input rows, odd columns), 1 = B (odd, even), 2 = C (even, odd), 3 = D (even, even).
    // Plane row y of an odd-row plane is input row 2 y - 1 (y = 0: the padding row), of an even-row plane input row 2 y.
    __host__ __device__ static constexpr int py(int pl) { return pl < 2 ? 1 : 0; }
    __host__ __device__ static constexpr int px(int pl) { return (pl == 0 || pl == 2) ? 1 : 0; }
    __host__ __device__ static constexpr int rows(int pl) { return TW + py(pl); }
    __host__ __device__ static constexpr int cols(int pl) { return TW + px(pl); }                 // = cell pitch
    __host__ __device__ static constexpr int cells(int pl) { return IMGS * rows(pl) * cols(pl); }
    static constexpr int A_PAD = (cells(0) + 127) / 128 * 128;                                    // plane A ends on a piece boundary
    __host__ __device__ static constexpr int cell0(int pl) {
        return pl == 0 ? 0 : A_PAD + (pl >= 2 ? cells(1) : 0) + (pl >= 3 ? cells(2) : 0);
    }
    static constexpr int TOTAL = cell0(3) + cells(3);
    static constexpr int NPT = (TOTAL + 127) / 128;               // pieces (= DMA instructions per thread and chunk): 11 | 10 | 10
    __host__ __device__ static constexpr int plane_of(int cell) { return cell < A_PAD ? 0 : (cell < cell0(2) ? 1 : (cell < cell0(3) ? 2 : 3)); }
    __host__ __device__ static constexpr int lo(int k) { return plane_of(128 * k); }
    __host__ __device__ static constexpr int hi(int k) { return plane_of(128 * k + 127 < TOTAL ? 128 * k + 127 : TOTAL - 1); }
    __host__ __device__ static constexpr int count_hi_le(int pl) { int n = 0; for (int k = 0; k < NPT; ++k) n += hi(k) <= pl ? 1 : 0; return n; }
    static constexpr int NA = count_hi_le(0);                     // pieces that hold plane A only
    static constexpr int PRO = count_hi_le(1);                    // ... planes A / B only: loaded ahead (prologue, next chunk)
    static constexpr int NB = PRO - NA;
    static constexpr int NOWN = NPT - PRO;                        // pieces with C / D cells: loaded in their own chunk's period
    // K-step (0..8 of a chunk's period) in which piece k is issued.  A pieces (next chunk): steps 5, 6 (masked input: all in
    // step 5: they must be readable LAND = 4 steps later, in step 0); B pieces (next chunk): steps 7, 8; own-period pieces:
    // one per step from step 0.
    __host__ __device__ static constexpr int pstep(int k) {
        return k < NA ? (!MSK ? 5 + (2 * k) / NA : 5) : (k < PRO ? 7 + (2 * (k - NA)) / NB : k - PRO);
    }
    __host__ __device__ static constexpr int pieces_at(int s) { int n = 0; for (int k = 0; k < NPT; ++k) n += pstep(k) == s ? 1 : 0; return n; }
    // Validity of that schedule (see the hazard notes in the kernel): a plane last read in step L may be overwritten from
    // step L + 2 on; a piece issued in step s has landed for every wave at the end of step s + NST - 1.
    __host__ __device__ static constexpr bool schedule_ok() {
        constexpr int first[4] = {0, 4, 6, 8}, last[4] = {3, 5, 7, 8};
        for (int k = 0; k < NPT; ++k) {
            const int s = pstep(k);
            if (k < PRO) {            // carries the NEXT chunk: period steps 9 + first[lo] is the deadline
                if (s < last[hi(k)] + 2 || s > 8 || s + LAND > 9 + first[lo(k)]) return false;
            } else {                  // carries its own chunk; the plane was last read in the previous period
                if (s + 9 < last[hi(k)] + 2 || s + LAND > first[lo(k)] || s > 4) return false;
            }
        }
        for (int s = 0; s < 9; ++s)
            if (pieces_at(s) > 3) return false;
        return NOWN <= 5 && NA >= 1 && NB >= 1;
    }
    static_assert(schedule_ok(), "patch refill schedule violates a WAR / RAW window");
    // DMA instructions of step s of a chunk (`last`: the tile's last chunk — no next-chunk pieces, no weights beyond the tile)
    __host__ __device__ static constexpr bool w_issued(int s, bool last) { return s + NST - 1 <= 8 || !last; }
    // keep-bit DMAs (MSK): one per piece, issued with it.  (One DMA for the bits of four pieces — three per chunk instead of ten — measured
    // slower, 2.21 -> 2.37 ms on the headline's pair launch: profiles/HISTORY.md.)
    __host__ __device__ static constexpr int bits_at(int s, bool last) { return MSK && (s <= 4 || !last) ? pieces_at(s) : 0; }
    __host__ __device__ static constexpr int p_issued(int s, bool last) { return ((s <= 4 || !last) ? pieces_at(s) : 0) + bits_at(s, last); }
    // What may still be in flight when step S ends: everything issued BEHIND the weights of step S + 1 (which were issued first
    // thing in step S - (NST - 2)): that step's pieces, then weights + pieces of the steps up to S.  (Steps before 0 are the
    // previous chunk's, never a last one; in a tile's first chunk they do not exist and the count is merely generous: the
    // prologue has waited for everything the first NST - 1 steps read.)
    __host__ __device__ static constexpr int wait_n(int S, bool last) {
        int n = 0;
        for (int j = S - (NST - 2); j <= S; ++j) {
            const bool prev = j < 0;
            const int sj = prev ? j + 9 : j;
            const bool lastj = last && !prev;
            if (j > S - (NST - 2)) n += w_issued(sj, lastj) ? WPI : 0;
            n += p_issued(sj, lastj);
        }
        return n;
    }
    static constexpr int WST = CT * 64;                           // one weight stage (32-deep K-step)
    static constexpr int PIECE = 512 * 16;
    static constexpr int P_OFF = (NST - 1) * WST;                 // [W0 | W1 | pieces ... | (pad) | last stage | BN]
    static constexpr int E_OFF = P_OFF + PRO * PIECE;             // pooled-exchange staging: the own-period pieces, padding, the last stage
    static constexpr int E_BYTES = 65536;
    static constexpr int END_PIECES = P_OFF + NPT * PIECE;
    static constexpr int WL_OFF = (END_PIECES + WST > E_OFF + E_BYTES ? END_PIECES : E_OFF + E_BYTES - WST);
    static constexpr int BN_OFF = WL_OFF + WST;
    static constexpr int BITS_OFF = BN_OFF + 2 * BN_MAX * 4 + 128;      // (behind the two image-row tables of the dynamic-exit instantiation)
    // keep-bit slots (2 KB: a dword per lane) of the pieces in flight.  A slot is live from the piece's issue to its masking three
    // steps later: own-period pieces (steps 0-4 -> 3-7) take slots 0-4, the A pieces (step 5 -> 8) slots 0, 1, 5, the B pieces
    // (steps 7, 8 -> 1, 2 of the next period) slots 2, 3.
    __host__ __device__ static constexpr int first_due(int S) {       // first piece whose masking is due in step S (issued in step S - 3 or S + 6), or -1
        for (int k = 0; k < NPT; ++k)
            if (pstep(k) + 3 == S || pstep(k) + 3 == S + 9) return k;
        return -1;
    }
    static constexpr int NSLOT = MSK ? 6 : 0;
    __host__ __device__ static constexpr int slot(int k) { return k >= PRO ? k - PRO : (k < NA ? (k < 2 ? k : 5) : 2 + (k - NA)); }
    static_assert(!MSK || (NA == 3 && NB == 2 && NOWN == 5 && NPT == 10), "keep-bit slot plan");
    // MSK: the four dword masks of a keep byte come from a 256-entry table (one ds_read_b128 instead of 16 vector instructions; with the
    // ds_and_b64 clear the pair launch of the headline 2.245 -> 2.18 ms, profiles/experiments/r3_lazy_site.log)
    static constexpr int LUT_OFF = BITS_OFF + NSLOT * 2048;
    static constexpr int LDS_BYTES = LUT_OFF + (MSK ? 4096 : 0);
    static_assert(BN_OFF - E_OFF >= E_BYTES, "epilogue staging area");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS");
    __host__ __device__ static constexpr int wstage_off(int st) { return st == NST - 1 ? WL_OFF : st * WST; }
    // tile pixel p -> image of the tile and output coordinates: the 16 pixels of one MFMA tile are a 4 x 4 block
    __host__ __device__ static constexpr int p_img(int p) { return p / (TW * TW); }
    __host__ __device__ static constexpr int p_ox(int p) { return 4 * ((p >> 4) % (TW / 4)) + (p & 3); }
    __host__ __device__ static constexpr int p_oy(int p) { return 4 * (((p >> 4) / (TW / 4)) % (TW / 4)) + ((p >> 2) & 3); }
    static constexpr int BR = TW / 4, BI = BR * BR;
    // cell of the j-th 4 x 4 block of a wave (its 8 blocks start at a multiple of 8) relative to the wave's first one, plane pl
    __host__ __device__ static constexpr int cell_delta(int pl, int j) {
        return (j / BI) * rows(pl) * cols(pl) + 4 * ((j % BI) / BR) * cols(pl) + 4 * ((j % BI) % BR);
    }
};

// step s of a chunk's period -> plane, cell shift (dy, dx) inside the plane, tap index ky * 3 + kx (weight offset)
__host__ __device__ constexpr int s2_plane(int s) { return s < 4 ? 0 : (s < 6 ? 1 : (s < 8 ? 2 : 3)); }
__host__ __device__ constexpr int s2_dy(int s) { return (s == 2 || s == 3 || s == 5) ? 1 : 0; }
__host__ __device__ constexpr int s2_dx(int s) { return (s == 1 || s == 3 || s == 7) ? 1 : 0; }
__host__ __device__ constexpr int s2_tap(int s) {
    constexpr int t[9] = {0, 2, 6, 8, 1, 7, 3, 5, 4};
    return t[s];
}

// The pad-skip tile order of the 8x8 -> 4x4 class ("s2_pad_skip", see the header comment): tile pixel p = 128 wp + 16 j + image, pixel tile j of
// pixel wave wp is the output position (oy, ox) = (j >> 1, 2 (j & 1) + ((oy + wp) & 1)) — conv3x3_pw's checkerboard (PwGeomSkip).  Step S
// (tap (ky, kx) = s2_tap(S)) of tile (wp, j) reads plane cell (oy + dy, ox + dx) of all 16 images, or — ky == 0 in output row 0, kx == 0 in
// output column 0 — nothing but the padding row / column of its plane.
struct S2Skip {
    __host__ __device__ static constexpr int t_y(int j) { return j >> 1; }
    __host__ __device__ static constexpr int t_x(int wp, int j) { return 2 * (j & 1) + (((j >> 1) + wp) & 1); }
    __host__ __device__ static constexpr bool valid(int wp, int j, int S) {
        return !((s2_tap(S) / 3 == 0 && t_y(j) == 0) || (s2_tap(S) % 3 == 0 && t_x(wp, j) == 0));
    }
    // cell (position) of the plane that the tile reads in step S: a multiple of 1 KB on the per-lane fragment address
    __host__ __device__ static constexpr int cell(int wp, int j, int S) {
        return (t_y(j) + s2_dy(S)) * (4 + ((s2_plane(S) & 1) ? 0 : 1)) + t_x(wp, j) + s2_dx(S);
    }
    __host__ __device__ static constexpr int count(int wp, int S) { int n = 0; for (int t = 0; t < 8; ++t) n += valid(wp, t, S) ? 1 : 0; return n; }
    // the live tiles of a K-step are split over its two phases in tile order (8: 4 + 4, 6: 3 + 3, 5: 3 + 2, 4: 2 + 2), as PwGeomSkip::phase
    __host__ __device__ static constexpr int phase(int wp, int j, int S) {
        int r = 0;
        for (int t = 0; t < j; ++t) r += valid(wp, t, S) ? 1 : 0;
        return r < (count(wp, S) + 1) / 2 ? 0 : 1;
    }
    __host__ __device__ static constexpr bool live(int wp, int j, int S, int kk) { return valid(wp, j, S) && phase(wp, j, S) == kk; }
    // bit j: tile j is live in phase kk of step S.  (The kernel takes the masks as constexpr values: left as calls with the unrolled tile index
    // for an argument, the two bodies of nine steps exhaust the inliner and real calls stay behind — around MFMAs, which ignore EXEC.)
    __host__ __device__ static constexpr unsigned mask(int wp, int S, int kk) { unsigned m = 0; for (int j = 0; j < 8; ++j) m |= live(wp, j, S, kk) ? 1u << j : 0u; return m; }
    __host__ __device__ static constexpr int sum(int wp) { int n = 0; for (int s = 0; s < 9; ++s) n += count(wp, s); return n; }
    __host__ __device__ static constexpr int slower() { int n = 0; for (int s = 0; s < 9; ++s) n += count(0, s) > count(1, s) ? count(0, s) : count(1, s); return n; }
    __host__ __device__ static constexpr bool cells_ok() {       // no live tile reads a padding cell or leaves its plane
        for (int wp = 0; wp < 2; ++wp)
            for (int j = 0; j < 8; ++j)
                for (int s = 0; s < 9; ++s) {
                    const int pl = s2_plane(s), y = t_y(j) + s2_dy(s), x = t_x(wp, j) + s2_dx(s);
                    const bool pad = (pl < 2 && y == 0) || ((pl == 0 || pl == 2) && x == 0);
                    if (valid(wp, j, s) == pad) return false;
                    if (y >= S2Geom<4>::rows(pl) || x >= S2Geom<4>::cols(pl) || cell(wp, j, s) != y * S2Geom<4>::cols(pl) + x) return false;
                }
        return true;
    }
};
static_assert(S2Skip::slower() == 61 && S2Skip::sum(0) + S2Skip::sum(1) == 121, "pad-skip: 61 of 72 tile-steps per chunk on the slower pixel wave, 121 of 144 live (position, tap) pairs");
static_assert(S2Skip::count(0, 0) == 5 && S2Skip::count(1, 0) == 4 && S2Skip::count(0, 8) == 8 && S2Skip::count(1, 4) == 6, "pad-skip: live tiles per tap");
static_assert(S2Skip::cells_ok(), "pad-skip: a tile is dead exactly when it reads the padding row / column of its plane");

// (the kernel's body: SKIP = the pad-skip form; the two entry points are below)
template <int TW, bool BF, bool IMAP, bool MSK, int CT_, bool SKIP>
__device__ __forceinline__ void conv3x3_s2_body(const ConvArgs& a, int n_tiles) {
    using G = S2Geom<TW, MSK, CT_>;
    static_assert(!MSK || (TW == 16 && !IMAP), "masked input: one image per tile, the ordinary form");
    static_assert(!SKIP || (TW == 4 && CT_ == 256 && !IMAP && !MSK), "pad-skip: the 8x8 -> 4x4 class without a row table");
    constexpr int CT = G::CT, IMGS = G::IMGS, NPT = G::NPT, PRO = G::PRO, NST = G::NST;
    constexpr bool HALF = CT == 128;
    constexpr int TI = 4, TP = HALF ? 4 : 8, JB = TP / 2;        // JB pixel blocks per phase of a K-step
    constexpr int PIECE_PHASE = 1;     // phase of a K-step whose LOAD part issues the step's patch pieces (phase 0 carries 8 fragment reads and
                                       // the 2 weight DMAs, phase 1 only 4 reads)
    typedef float accv __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(16))) char smem[G::LDS_BYTES];
    char* const pbuf = smem + G::P_OFF;
    float* const bn_scale = (float*)(smem + G::BN_OFF);
    float* const bn_bias = bn_scale + G::BN_MAX;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15, kq = lane >> 4;
    const int g = wave >> 2, wc = (wave >> 1) & 1, wp = wave & 1;

    const int n_ctiles = a.Cout / CT;
    const int n_ptiles = (a.N + IMGS - 1) / IMGS;
    const int Ktot = 9 * a.Cin;
    const int nC = a.Cin / 32;
    const int split = a.wgt_b ? a.split : a.Cout;

    // folded-BN table of the whole launch (an ordinary global load inside the epilogue would make hipcc drain the LDS-DMA)
    for (int c = tid; c < a.Cout; c += 512) {
        const bool second = c >= split;
        const float* sp = second ? a.scale_b : a.scale;
        const float* bp = second ? a.bias_b : a.bias;
        const int cc = second ? c - split : c;
        bn_scale[c] = (sp ? sp[cc] : 1.f) * a.out_mul;
        bn_bias[c] = bp ? bp[cc] : 0.f;
    }
    if constexpr (MSK) {
        if (tid < 256) {
            typedef unsigned int u32x4_l __attribute__((ext_vector_type(4)));
            u32x4_l m;
#pragma unroll
            for (int i = 0; i < 4; ++i) m[i] = (((tid >> (2 * i)) & 1) ? 0xffffu : 0u) | (((tid >> (2 * i + 1)) & 1) ? 0xffff0000u : 0u);
            *(u32x4_l*)(smem + G::LUT_OFF + tid * 16) = m;
        }
    }
    __syncthreads();   // (no LDS-DMA in flight yet: the plain barrier and its waits are fine here)

    // ---- per-lane fragment geometry (tile-independent) ----
    // weights: row (g*128 + wc*64 + l16 + 16 i), chunk kq at position kq ^ 2 ((row >> 2) & 1) = kq ^ 2 ((l16 >> 2) & 1)
    // (the parentheses around the lane's row are conv3x3_pw's, where they shape the instruction order: keep)
    const int a_off = ((HALF ? 0 : g * 128) + wc * 64 + (8 * (l16 >> 2) + (l16 & 3))) * 64 + ((kq ^ (((l16 >> 2) & 1) << 1)) << 4);
    // byte offset of channel tile i's row of this lane relative to a_off
#define A_TILE(I) ((32 * ((I) >> 1) + 4 * ((I) & 1)) * 64)
    // pixels: lane (by, bx) = (l16 >> 2, l16 & 3) of each 4 x 4 block; plane row parity of the cell = (by + dy) & 1
    const int by = l16 >> 2, bx = l16 & 3;
    const int pbase = HALF ? (g * 2 + wp) * 64 : wp * 128;        // first tile pixel of this wave
    // (a tap with dy = 1 reads the cell one plane row further down: + cols * 64 as an immediate, and the chunk sits at the
    // other position of its pair: the same per-lane address with bit 5 flipped)
    int boff[4];
#pragma unroll
    for (int pl = 0; pl < 4; ++pl) {
        const int wave_cell = G::cell0(pl) + (G::p_img(pbase) * G::rows(pl) + G::p_oy(pbase)) * G::cols(pl) + G::p_ox(pbase);
        boff[pl] = G::P_OFF + (wave_cell + by * G::cols(pl) + bx) * 64 + ((kq ^ ((by & 1) << 1)) << 4);
        // pad-skip: lane l16 is IMAGE l16 of the cell the tile reads; the cell (tile position + tap shift) is an immediate multiple of 1 KB
        if constexpr (SKIP) boff[pl] = G::P_OFF + (G::cell0(pl) + l16) * 64 + ((kq ^ (((l16 >> 3) & 1) << 1)) << 4);
    }

    // ---- per-thread DMA sources ----
    // Every DMA is a buffer_load ... lds through a per-tile buffer descriptor (wave-uniform, SGPRs) with a 32-bit per-lane byte
    // offset: no 64-bit address arithmetic or pointer selects in the loop, and a lane whose offset lies beyond the descriptor's
    // size loads ZEROS — the padding ring of the patch, the cells behind a plane, the images of a last tile beyond N.
    // patch: piece q = tid + 512 k -> cell q >> 2 of the piece array, position q & 3 holds chunk (q & 3) ^ 2 (y & 1).  What a
    // piece reads is the same for every tile up to the tile's first image: pre[k] = byte offset of the piece's source
    // relative to image n0 of the input (2 (img * H*W*Cin + (iy * W + ix) * Cin + chunk * 8)), computed ONCE per kernel; the
    // descriptor of a tile starts at its image n0 and ends behind its last image.  (IMAP: the images of a tile are not
    // consecutive rows — pre[k] = img << 24 | in-image ELEMENT offset, the rows come from a per-tile LDS table and the
    // descriptor covers the whole tensor.)
    const unsigned HWC = (unsigned)a.H * a.W * a.Cin;             // (launcher: N <= in_mod, in_mod * HWC < 2^31, HWC < 2^24)
    constexpr unsigned OOB = 0xfffffff0u;                         // beyond every descriptor (a tile's <= 16 images; IMAP: the tensor, < 2^32 - 16 bytes)
    unsigned pre[NPT];
#pragma unroll
    for (int k = 0; k < NPT; ++k) {
        const int q = tid + 512 * k;
        const int cell = q >> 2, pos = q & 3;
        const int pl = G::lo(k) == G::hi(k) ? G::lo(k) : (cell < G::cell0(G::hi(k)) ? G::lo(k) : G::hi(k));
        const int pyl = pl < 2 ? 1 : 0, pxl = (pl == 0 || pl == 2) ? 1 : 0;
        const int RQ = (TW + pyl) * (TW + pxl), Q = TW + pxl;
        const int lc = cell - (pl == 0 ? 0 : (pl == 1 ? G::cell0(1) : (pl == 2 ? G::cell0(2) : G::cell0(3))));
        // (pad-skip: the cells of a plane are numbered (y * cols + x) * 16 + img, the image fastest: a pixel fragment = 16 images of one cell = 1 KB)
        const int img = SKIP ? (lc & 15) : lc / RQ, rm = SKIP ? (lc >> 4) : lc - img * RQ;
        const int y = rm / Q, x = rm - y * Q;
        const int iy = 2 * y - pyl, ix = 2 * x - pxl;
        const int sw = SKIP ? ((img >> 3) & 1) : (y & 1);        // chunk swizzle: pos ^ 2 sw
        const bool ok = lc < IMGS * RQ && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
        // (masked input in the lazy site's planar layout, kernels.h lazy_planar_off: a plane row's cells are contiguous 64-byte runs)
        const unsigned inoff = (MSK && a.lazy_planar) ? (unsigned)((iy * a.W + (ix & 1) * (a.W >> 1) + (ix >> 1)) * 32 + ((pos ^ (sw << 1)) << 3))
                                                      : (unsigned)((iy * a.W + ix) * a.Cin + ((pos ^ (sw << 1)) << 3));
        pre[k] = !ok ? OOB : (IMAP ? ((unsigned)img << 24) | inoff : 2u * ((unsigned)img * HWC + inoff));
    }
    // IMAP: tensor row of each image of a tile (-1 beyond N), two tables: the epilogue of tile i reads table i & 1 while the
    // prologue of tile i + 1 is issued from table (i + 1) & 1
    int* const row_tabs = (int*)(smem + G::BN_OFF + 2 * G::BN_MAX * 4);
    int tsel = 0;
    // weights: piece q = tid + 512 i -> row (tid >> 2) + 128 i, position tid & 3 holds chunk (tid & 3) ^ 2 ((row >> 2) & 1);
    // one descriptor per 128-row half of the channel tile (a pair's second conv has its own weight tensor)
    // (the MFMA row permutation: a fragment's 16 lanes read rows 8 a + b + const, so the chunk position alternates with row >> 3 instead of row >> 2)
    const unsigned woff = 2u * ((unsigned)(tid >> 2) * Ktot + (((tid & 3) ^ (((tid >> 5) & 1) << 1)) << 3));
    const unsigned wbytes = 2u * 128u * Ktot;
    // element offset of channel chunk C0 (a multiple of 32) = C0 * cmul: 1 in NHWC, H * W in the planar layout (one 32-channel plane per chunk)
    const unsigned cmul = (MSK && a.lazy_planar) ? (unsigned)(a.H * a.W) : 1u;
    __amdgpu_buffer_rsrc_t rs_w0, rs_w1, rs_in, rs_bits;

    int ch0 = 0, n0 = 0;

    // (the K offset of a step — tap and channel chunk, wave-uniform — rides in the instruction's SGPR offset: the per-lane
    // offsets stay loop-invariant, one VGPR each, and nothing is added per DMA)
#define BLDS16(RSRC, VOFF, SOFF, LDSPTR) \
    __builtin_amdgcn_raw_ptr_buffer_load_lds((RSRC), (__attribute__((address_space(3))) void*)(LDSPTR), 16, (VOFF), (SOFF), 0, 0)
#define ISSUE_W(KOFF, ST)                                                                                    \
    {                                                                                                        \
        const unsigned so_ = __builtin_amdgcn_readfirstlane(2u * (unsigned)(KOFF));                          \
        BLDS16(rs_w0, woff, so_, smem + G::wstage_off(ST) + (0 * 512 + wave * 64) * 16);                     \
        if (!HALF) BLDS16(rs_w1, woff, so_, smem + G::wstage_off(ST) + (1 * 512 + wave * 64) * 16);          \
    }
#define ISSUE_P(K, C0)                                                                                       \
    {                                                                                                        \
        unsigned o_ = pre[K];                                                                                \
        if constexpr (IMAP) {                                                                                \
            const int row_ = row_tabs[tsel * 16 + ((pre[K] >> 24) & 15)];                                    \
            o_ = (pre[K] == OOB || row_ < 0) ? OOB : 2u * ((unsigned)row_ * HWC + (pre[K] & 0xffffffu));     \
        }                                                                                                    \
        BLDS16(rs_in, o_, __builtin_amdgcn_readfirstlane(2u * (unsigned)(C0) * cmul), pbuf + ((K) * 512 + wave * 64) * 16); \
        if constexpr (MSK) {                                                                                 \
            /* the cell's 32 keep bits of this chunk (the dword that holds this piece's byte); beyond the descriptor: zeros */ \
            /* (derived from pre[K] at every issue: as loop invariants the ten offsets are spilled, and a scratch reload in */ \
            /*  front of a DMA is a vmcnt wait for everything in flight)                                                    */ \
            unsigned bo_ = pre[K];                                                                           \
            asm volatile("" : "+v"(bo_));                                                                    \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_bits, (__attribute__((address_space(3))) void*)(smem + G::BITS_OFF + G::slot(K) * 2048 + wave * 256), \
                                                     4, (bo_ >> 4) & ~3u, __builtin_amdgcn_readfirstlane(((unsigned)(C0) * cmul) >> 3), 0, 0); \
        }                                                                                                    \
    }
    // The thread that issued piece K clears the dropped elements of its 16 bytes: byte (logical chunk) of the slot's dword -> four
    // dword masks.  Own DMA only: the thread's counted vmcnt wait is all it needs; the barriers of the step publish the result.
    typedef unsigned int u32x4_m __attribute__((ext_vector_type(4)));
#define MASK_LOAD(K, W)                                                                                      \
    {                                                                                                        \
        int t4_ = tid * 4;                                                                                   \
        asm volatile("" : "+v"(t4_));                                                                        \
        W = *(const unsigned*)(smem + G::BITS_OFF + G::slot(K) * 2048 + t4_);                                /* the dword of this piece's cell */ \
    }
    // (two ds_and_b64: the LDS unit reads, ANDs and writes — no round trip through the registers)
#define MASK_STORE(K, W)                                                                                     \
    {                                                                                                        \
        unsigned sh_ = pre[K];                                                                               \
        asm volatile("" : "+v"(sh_));                                                                        \
        const int b_ = (int)((W) >> ((sh_ >> 1) & 24u));                                                     \
        const u32x4_m m_ = *(const u32x4_m*)(smem + G::LUT_OFF + ((b_ & 0xff) << 4));                        \
        typedef __attribute__((address_space(3))) unsigned long long lds_u64;                                \
        lds_u64* const q_ = (lds_u64*)(pbuf + ((K) * 512 + tid) * 16);                                       \
        __atomic_fetch_and(q_, ((unsigned long long)m_[1] << 32) | m_[0], __ATOMIC_RELAXED);                 \
        __atomic_fetch_and(q_ + 1, ((unsigned long long)m_[3] << 32) | m_[2], __ATOMIC_RELAXED);             \
    }
#define MASK_P(K)                                                                                            \
    {                                                                                                        \
        unsigned mw_;                                                                                        \
        MASK_LOAD(K, mw_);                                                                                   \
        MASK_STORE(K, mw_);                                                                                  \
    }
    // piece whose masking is due in step S of a period (issued three steps earlier), -1: none.  (Step 8: the A pieces, all three
    // issued in step 5: the first one takes the early-load slot, the others follow serially.)
#define MASK_DUE(S, K) (G::pstep(K) + 3 == (S) || G::pstep(K) + 3 == (S) + 9)
    // Tile VB: its buffer descriptors; its first two weight stages and the pieces that hold planes A / B only (chunk 0) are
    // issued: everything the first K-steps read.
#define SETUP_TILE(VB)                                                                                       \
    {                                                                                                        \
        int ptile_, ctile_;                                                                                  \
        if (MSK && a.lazy_order) {          /* position = id ((b T + t) n_ct + ct): sample-minor, one image per tile */ \
            const unsigned T_ = (unsigned)(a.N / a.in_mod), r_ = (unsigned)(VB) / (unsigned)n_ctiles;       \
            ctile_ = (int)((unsigned)(VB) - r_ * (unsigned)n_ctiles);                                        \
            const unsigned b_ = r_ / T_;                                                                     \
            ptile_ = (int)((r_ - b_ * T_) * (unsigned)a.in_mod + b_);                                        \
        } else {                                                                                             \
            xcd_tile_map((VB), n_ptiles, n_ctiles, ptile_, ctile_, a.xcd_split);                             \
        }                                                                                                    \
        ch0 = ctile_ * CT;                                                                                   \
        n0 = ptile_ * IMGS;                                                                                  \
        const _Float16* w0_ = ch0 < split ? a.wgt + (size_t)ch0 * Ktot : a.wgt_b + (size_t)(ch0 - split) * Ktot; \
        const _Float16* w1_ = ch0 + 128 < split ? a.wgt + (size_t)(ch0 + 128) * Ktot : a.wgt_b + (size_t)(ch0 + 128 - split) * Ktot; \
        rs_w0 = __builtin_amdgcn_make_buffer_rsrc((void*)w0_, 0, wbytes, 0x00020000);                        \
        if (!HALF) rs_w1 = __builtin_amdgcn_make_buffer_rsrc((void*)w1_, 0, wbytes, 0x00020000);             \
        if constexpr (IMAP) {                                                                                \
            rs_in = __builtin_amdgcn_make_buffer_rsrc((void*)a.in, 0, 2u * (unsigned)a.in_mod * HWC, 0x00020000); \
        } else {                                                                                             \
            const int nimg_ = a.N - n0 < IMGS ? a.N - n0 : IMGS;                                             \
            /* (one image per tile: a deterministic input of in_mod images serves every sample; launcher: in_mod >= N otherwise) */ \
            const int row0_ = IMGS == 1 ? n0 % a.in_mod : n0;                                                \
            rs_in = __builtin_amdgcn_make_buffer_rsrc((void*)(a.in + (size_t)row0_ * HWC), 0, 2u * (unsigned)nimg_ * HWC, 0x00020000); \
            if constexpr (MSK)                                                                               \
                rs_bits = __builtin_amdgcn_make_buffer_rsrc((void*)(a.in_bits + (size_t)n0 * (HWC >> 3)), 0, HWC >> 3, 0x00020000); \
        }                                                                                                    \
        ISSUE_W(0, 0);                                                                                       \
        if constexpr (IMAP) {                                                                                \
            tsel ^= 1;                                                                                       \
            if (tid < IMGS) row_tabs[tsel * 16 + tid] = n0 + tid < a.N ? a.imap[n0 + tid] : -1;              \
            __syncthreads();   /* (drains W(0) too: the dynamic-exit path only) */                           \
        }                                                                                                    \
        _Pragma("unroll") for (int k = 0; k < PRO; ++k) ISSUE_P(k, 0);                                       \
        ISSUE_W(s2_tap(1) * a.Cin, 1);                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                                                   \
    }

#define RAW_BARRIER()                                  \
    {                                                  \
        __builtin_amdgcn_sched_barrier(0);             \
        asm volatile("" ::: "memory");                 \
        __builtin_amdgcn_s_barrier();                  \
        asm volatile("" ::: "memory");                 \
        __builtin_amdgcn_sched_barrier(0);             \
    }
#define WAIT_VM(N) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory")
    // What may still be in flight when K-step S of a chunk ends: the weight tile of the step after next (2 DMA instructions,
    // issued this step) and the patch pieces issued this step and the step before; everything older — in particular the next
    // step's weights and every piece issued two or more steps ago — has landed.  In the last chunk no next-chunk piece (steps
    // 5-8) and no weights beyond the tile's last step (steps 7, 8) are issued.
    // (Letting the previous tile's output stores stay in flight through step 0 of the next tile was built and measured neutral, +-0.5 %, in
    //  round 4: the tile-start wait below drains them.)
#define END_OF_STEP_WAIT(S)                                                                                    \
    {                                                                                                          \
        if (!last) { WAIT_VM(G::wait_n(S, false)); }                                                           \
        else { WAIT_VM(G::wait_n(S, true)); }                                                                  \
    }
    // One K-step = step S of the chunk's period (one tap x this chunk's 32 channels).  Two phases (LOAD part, barrier, MFMA part,
    // barrier); the two wave groups run one barrier apart.  Weight stage = S % 3 (9 steps per chunk: the index repeats).
    // Intervals between barriers, global step T: group 0 LOAD 4T+2k, MFMA 4T+2k+1; group 1 one later.
    //   WAR  weight stage (T+2)%3 was last read in 4T-3 (group 1, phase 0 of T-1; retired by its lgkmcnt(0) in 4T-2): refilled
    //        from 4T on.  A patch plane last read in step L (group 1's phase-1 reads retire in 4L+4) is refilled from step L+2.
    //   RAW  in interval 4T+3 every wave waits (counted vmcnt) until only the DMA of steps T and the pieces of T-1 are in flight.
#define S2_STEP(S)                                                                                             \
    {                                                                                                          \
        constexpr int pl_ = s2_plane(S), dy_ = s2_dy(S), dx_ = s2_dx(S), sn_ = (S) + NST - 1;                  \
        /* stage read by this step / filled for step S + NST - 1: compile-time (9 steps per chunk: the index repeats) */ \
        constexpr int st_r_ = (S) % 3, st_w_ = ((S) + 2) % 3;                                                  \
        const char* ws_ = smem + G::wstage_off(st_r_) + a_off;                                                 \
        const char* pb_ = smem + (dy_ * G::cols(pl_) + dx_) * 64 + (boff[pl_] ^ (dy_ << 5));                   \
        /* MSK: pieces issued three steps ago have landed (this thread's wait at the end of the previous step).  The first due */ \
        /* piece is read BEFORE the fragment reads and finished behind them: its LDS round trip overlaps their issue — as one  */ \
        /* serial read-modify-write in front of them it stretched the LOAD part past the other group's MFMA part (2.03 -> 2.26 ms */ \
        /* on the 64 -> 128+128 launch of the headline) */                                                     \
        constexpr int due0_ = G::first_due(S);                                                                 \
        const bool due_on_ = MSK && due0_ >= 0 && (due0_ >= PRO ? true : (G::pstep(due0_ < 0 ? 0 : due0_) + 3 == (S) ? !last : chunk > 0)); \
        unsigned mw0_ = 0;                                                                                     \
        _Pragma("unroll") for (int kk = 0; kk < 2; ++kk) {                                                     \
            if constexpr (MSK && due0_ >= 0) { if (kk == 0 && due_on_) { MASK_LOAD(due0_ < 0 ? 0 : due0_, mw0_); } } \
            if (kk == 0) {                                                                                     \
                _Pragma("unroll") for (int i = 0; i < TI; ++i) af[i] = *(const half8*)(ws_ + A_TILE(i));       \
            }                                                                                                  \
            _Pragma("unroll") for (int j = 0; j < JB; ++j)                                                     \
                bf[j] = *(const half8*)(pb_ + G::cell_delta(pl_, JB * kk + j) * 64);                           \
            if constexpr (MSK && due0_ >= 0) {                                                                 \
                if (kk == 0) {                                                                                 \
                    if (due_on_) { MASK_STORE(due0_ < 0 ? 0 : due0_, mw0_); }                                  \
                    _Pragma("unroll") for (int k = 0; k < NPT; ++k)                                            \
                        if (k != due0_ && MASK_DUE(S, k)) { if (due_on_) { MASK_P(k); } }                      \
                }                                                                                              \
            }                                                                                                  \
            if (kk == 0) {                                                                                     \
                /* weights of step S + NST - 1: of this chunk, or of the first steps of the next one */        \
                if (sn_ <= 8) { ISSUE_W(s2_tap(sn_ <= 8 ? sn_ : 0) * a.Cin + c32, st_w_); }                    \
                else if (!last) { ISSUE_W(s2_tap(sn_ > 8 ? sn_ - 9 : 0) * a.Cin + c32 + 32, st_w_); }          \
            }                                                                                                  \
            if (kk == PIECE_PHASE) {                                                                           \
                _Pragma("unroll") for (int k = 0; k < NPT; ++k)                                                \
                    if (G::pstep(k) == (S)) {                                                                  \
                        if (k >= PRO) { ISSUE_P(k, c32); }                                                     \
                        else if (!last) { ISSUE_P(k, c32 + 32); }                                              \
                    }                                                                                          \
            }                                                                                                  \
            if (kk == 1 && g == 1) END_OF_STEP_WAIT(S);        /* interval 4T+3, group 1: LOAD part */         \
            RAW_BARRIER();                                                                                     \
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                 \
            __builtin_amdgcn_s_setprio(1);                                                                     \
            _Pragma("unroll") for (int i = 0; i < TI; ++i)                                                     \
                _Pragma("unroll") for (int j = 0; j < JB; ++j)                                                 \
                    acc[i][JB * kk + j] = mfma_16x16x32<BF>(af[i], bf[j], acc[i][JB * kk + j]);                \
            __builtin_amdgcn_s_setprio(0);                                                                     \
            if (kk == 1 && g == 0) END_OF_STEP_WAIT(S);        /* interval 4T+3, group 0: MFMA part */         \
            RAW_BARRIER();                                                                                     \
        }                                                                                                      \
    }

    // The pad-skip K-step (S2_STEP without the masked-input parts): a phase reads and multiplies only the tiles that are live in it
    // (S2Skip::live, compile-time per pixel wave WP) — a dead tile is a ds_read_b128 and four MFMAs that are not emitted.  DMA issue, waits
    // and barriers are S2_STEP's.
#define S2_STEP_S(S, WP)                                                                                       \
    {                                                                                                          \
        constexpr int pl_ = s2_plane(S), sn_ = (S) + NST - 1;                                                  \
        constexpr int st_r_ = (S) % 3, st_w_ = ((S) + 2) % 3;                                                  \
        constexpr unsigned live_[2] = {S2Skip::mask(WP, S, 0), S2Skip::mask(WP, S, 1)};                        \
        constexpr int cols_ = G::cols(pl_), shift_ = s2_dy(S) * cols_ + s2_dx(S);       /* cell of tile j: its position + the tap shift */ \
        static_assert(S2Skip::cell(WP, 5, S) == (5 >> 1) * cols_ + 2 * (5 & 1) + (((5 >> 1) + (WP)) & 1) + shift_, "cell"); \
        const char* ws_ = smem + G::wstage_off(st_r_) + a_off;                                                 \
        const char* pb_ = smem + boff[pl_];                                                                    \
        _Pragma("unroll") for (int kk = 0; kk < 2; ++kk) {                                                     \
            if (kk == 0) {                                                                                     \
                _Pragma("unroll") for (int i = 0; i < TI; ++i) af[i] = *(const half8*)(ws_ + A_TILE(i));       \
            }                                                                                                  \
            _Pragma("unroll") for (int j = 0; j < TP; ++j)                                                     \
                if ((live_[kk] >> j) & 1u) bfs[j] = *(const half8*)(pb_ + ((j >> 1) * cols_ + 2 * (j & 1) + (((j >> 1) + (WP)) & 1) + shift_) * 1024); \
            if (kk == 0) {                                                                                     \
                if (sn_ <= 8) { ISSUE_W(s2_tap(sn_ <= 8 ? sn_ : 0) * a.Cin + c32, st_w_); }                    \
                else if (!last) { ISSUE_W(s2_tap(sn_ > 8 ? sn_ - 9 : 0) * a.Cin + c32 + 32, st_w_); }          \
            }                                                                                                  \
            if (kk == PIECE_PHASE) {                                                                           \
                _Pragma("unroll") for (int k = 0; k < NPT; ++k)                                                \
                    if (G::pstep(k) == (S)) {                                                                  \
                        if (k >= PRO) { ISSUE_P(k, c32); }                                                     \
                        else if (!last) { ISSUE_P(k, c32 + 32); }                                              \
                    }                                                                                          \
            }                                                                                                  \
            if (kk == 1 && g == 1) END_OF_STEP_WAIT(S);                                                        \
            RAW_BARRIER();                                                                                     \
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                 \
            __builtin_amdgcn_s_setprio(1);                                                                     \
            _Pragma("unroll") for (int i = 0; i < TI; ++i)                                                     \
                _Pragma("unroll") for (int j = 0; j < TP; ++j)                                                 \
                    if ((live_[kk] >> j) & 1u) acc[i][j] = mfma_16x16x32<BF>(af[i], bfs[j], acc[i][j]);        \
            __builtin_amdgcn_s_setprio(0);                                                                     \
            if (kk == 1 && g == 0) END_OF_STEP_WAIT(S);                                                        \
            RAW_BARRIER();                                                                                     \
        }                                                                                                      \
    }
#define S2_CHUNKS_S(WP)                                                                                        \
    for (int chunk = 0; chunk < nC; ++chunk) {                                                                 \
        const bool last = chunk + 1 == nC;                                                                     \
        const int c32 = chunk * 32;                                                                            \
        S2_STEP_S(0, WP) S2_STEP_S(1, WP) S2_STEP_S(2, WP) S2_STEP_S(3, WP) S2_STEP_S(4, WP)                   \
        S2_STEP_S(5, WP) S2_STEP_S(6, WP) S2_STEP_S(7, WP) S2_STEP_S(8, WP)                                    \
    }

    // The walk: tile positions blockIdx.x, + gridDim.x, ... through xcd_tile_map — or, reading a deterministic input through keep bits
    // (MSK, ConvArgs::lazy_order), the sample-minor numbering id = (b T + t) n_ct + ct dealt per XCD: XCD x (workgroups = x mod 8, J of
    // them) owns the contiguous ids [x L, (x + 1) L) and its workgroup j takes x L + j, + J, ...: at any moment the XCD's workgroups read
    // ONE image's patch (consecutive samples of it), which therefore stays in the XCD's 4 MB L2 — with a run of ids per WORKGROUP (first
    // version) 32 different images of 131-512 KB each pass through it and every sample's read is a miss again.
    int vb = blockIdx.x, v_step = (int)gridDim.x, v_end = n_tiles;
    if (MSK && a.lazy_order) {
        if ((gridDim.x & 7) == 0) {
            const int L = (n_tiles + 7) >> 3, J = (int)gridDim.x >> 3;
            vb = (int)(blockIdx.x & 7) * L + (int)(blockIdx.x >> 3);
            v_step = J;
            v_end = (int)((blockIdx.x & 7) + 1) * L < n_tiles ? (int)((blockIdx.x & 7) + 1) * L : n_tiles;
        }                                                   // (a grid that is not a multiple of eight — fewer tiles than CUs: the ids in order)
        if (vb >= v_end) return;
    }
    SETUP_TILE(vb);
    constexpr int NSTORES = HALF ? 8 : 16;                 // output stores per thread of a full tile
    bool stores16 = false;                                 // the tile before this one issued exactly NSTORES stores per thread
    [[maybe_unused]] bool pooled_prev = false;             // pad-skip: ... and this wave's channel half was pooled (4 stores in pixel wave 0, none in pixel wave 1)
    while (vb < v_end) {
        const int cur_ch0 = ch0, cur_n0 = n0, cur_tsel = tsel;
        accv acc[TI][TP];
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < TP; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.f;

        // weight stages 0, 1 and the A / B pieces of chunk 0 have landed.  The previous tile's 16 output stores per thread were
        // issued BEHIND them (vmcnt retires in order): a full tile leaves them in flight, a ragged one (some stores skipped:
        // the count is not known) and the dynamic-exit form drain everything.
        if (IMAP || !stores16) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else if (SKIP && pooled_prev) {                    // (wave-uniform: the count is per wave)
            if (wp) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        }
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NSTORES) : "memory");
        if constexpr (MSK) {                               // the A / B pieces of chunk 0 (issued by SETUP_TILE)
#pragma unroll
            for (int k = 0; k < PRO; ++k) MASK_P(k);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        RAW_BARRIER();
        if (g == 1) RAW_BARRIER();                         // stagger
        half8 af[TI];
        if constexpr (SKIP) {
            half8 bfs[TP];
            if (wp == 0) { S2_CHUNKS_S(0) } else { S2_CHUNKS_S(1) }      // (wave-uniform: both sides take the same barriers)
        } else {
            half8 bf[4];
            for (int chunk = 0; chunk < nC; ++chunk) {
                const bool last = chunk + 1 == nC;
                const int c32 = chunk * 32;
                S2_STEP(0) S2_STEP(1) S2_STEP(2) S2_STEP(3) S2_STEP(4) S2_STEP(5) S2_STEP(6) S2_STEP(7) S2_STEP(8)
            }
        }
        if (g == 0) RAW_BARRIER();                         // both groups aligned: every wave is done with the stages and the patch
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

        // ---- next tile's first weight stages and A / B pieces; they land during the epilogue below ----
        const int nvb = vb + v_step;
        if (nvb < v_end) SETUP_TILE(nvb);

        [[maybe_unused]] bool pooled_now = false;
        // ---- epilogue of the current tile: BN + ReLU on the accumulators, fp16 straight from the registers ----
        int tl = tid & 255;
        asm volatile("" : "+v"(tl));                        // (unused: kept only because it shapes register allocation — without it the SGPR-spill VGPR moves)
        const int chl = cur_ch0 + (HALF ? 0 : 128 * g);    // launch-wide channel of this group's channel 0 (BN table index)
        _Float16* outp = a.out;
        int oc = a.Cout, chg = chl;
        if (a.wgt_b) {
            if (chl >= split) { outp = a.out_b; oc = a.Cout - split; chg = chl - split; }
            else oc = split;
        }
        float* const poolp = TW == 4 ? ((a.wgt_b && chl >= split) ? a.pool_b : a.pool) : nullptr;     // wave-uniform (per channel half)
        if constexpr (SKIP) pooled_now = poolp != nullptr;
        if (SKIP && poolp) {
            if constexpr (SKIP) {
            // Pad-skip: an image's 16 positions are the 8 tile registers of this lane and of the same lane of the partner wave (wp ^ 1).  The sum
            // keeps the order of the DPP tree below — map row y: (p0 + p1) + (p2 + p3), then (r0 + r1) + (r3 + r2), then * 1/16 — through the staging
            // area at E_OFF, which nothing of the next tile touches before its step 0 (conv3x3_pw's persistent pooled tail): wave wp sends the tiles
            // of rows 2 (1 - wp), 2 (1 - wp) + 1 and sums rows 2 wp, 2 wp + 1 (a pair p0 + p1 / p2 + p3 is one value of each wave; float addition
            // commutes); pixel wave 1 then sends r2 + r3 and pixel wave 0 stores.  Slot of wave w: 8 KB, [tile 0..3][quad 0..1][lane] float4.
            // Three barriers per 32-channel half h: a channel group that stores plainly (mixed pair) takes the same six below.
            char* const X = smem + G::E_OFF;
            char* const mine_x = X + wave * 8192 + lane * 16;
            char* const theirs_x = X + (wave ^ 1) * 8192 + lane * 16;
            const int chw = chl + wc * 64 + 8 * kq;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                f32x4_e sc[2], bi[2];
#pragma unroll
                for (int ii = 0; ii < 2; ++ii) {
                    sc[ii] = *(const f32x4_e*)(bn_scale + chw + 32 * h + 4 * ii);
                    bi[ii] = *(const f32x4_e*)(bn_bias + chw + 32 * h + 4 * ii);
                }
                float xs[TP][8];                                      // relu(bn(.)) of this lane's 8 channels at its 8 positions
#pragma unroll
                for (int j = 0; j < TP; ++j)
#pragma unroll
                    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                        for (int e = 0; e < 4; ++e) xs[j][4 * ii + e] = fmaxf(__builtin_fmaf(acc[2 * h + ii][j][e], sc[ii][e], bi[ii][e]), 0.f);
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        f32x4_e t;
#pragma unroll
                        for (int e = 0; e < 4; ++e) t[e] = wp ? xs[jj][4 * q + e] : xs[4 + jj][4 * q + e];
                        *(f32x4_e*)(mine_x + (jj * 2 + q) * 1024) = t;
                    }
                lds_barrier();
                float rs[2][8];                                       // the two row sums of this wave
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const f32x4_e t0 = *(const f32x4_e*)(theirs_x + ((2 * r) * 2 + q) * 1024), t1 = *(const f32x4_e*)(theirs_x + ((2 * r + 1) * 2 + q) * 1024);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float o0 = wp ? xs[4 + 2 * r][4 * q + e] : xs[2 * r][4 * q + e], o1 = wp ? xs[4 + 2 * r + 1][4 * q + e] : xs[2 * r + 1][4 * q + e];
                            const float s01 = o0 + t0[e], s23 = o1 + t1[e];
                            rs[r][4 * q + e] = s01 + s23;
                        }
                    }
                float half_sum[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) half_sum[c] = rs[0][c] + rs[1][c];          // r0 + r1 | r2 + r3
                lds_barrier();                                        // every wave has read its partner's slot
                if (wp) {
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        f32x4_e t;
#pragma unroll
                        for (int e = 0; e < 4; ++e) t[e] = half_sum[4 * q + e];
                        *(f32x4_e*)(theirs_x + q * 1024) = t;
                    }
                }
                lds_barrier();
                if (!wp) {
                    const int n = cur_n0 + l16;
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        const f32x4_e t = *(const f32x4_e*)(mine_x + q * 1024);
                        f32x4_e pv;
#pragma unroll
                        for (int e = 0; e < 4; ++e) pv[e] = (half_sum[4 * q + e] + t[e]) * (1.f / 16.f);
                        if (n < a.N) *(f32x4_e*)(poolp + (size_t)n * oc + chg + wc * 64 + 8 * kq + 32 * h + 4 * q) = pv;
                    }
                }
            }
            // (the next tile's own-period pieces overwrite the staging area from its step 0: every exchange read is complete before the tile-start barrier)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
        } else if (poolp) {
            // ReLU + global average pool fused (the conv feeds an exit head only): a wave's pixel tile j is image wp * 8 + j of
            // the tile, its 16 pixels the 16 lanes of a DPP row — four v_add_f32 with DPP (quad xor 1, xor 2, half mirror, row
            // mirror) leave the sum in every lane; lane 0 of each row stores 4 consecutive channels as fp32.  Nothing goes
            // through LDS.
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int cw = 32 * (i >> 1) + 8 * kq + 4 * (i & 1);      // this lane's 4 channels of tile i
                const int c4 = chl + wc * 64 + cw;
                const f32x4_e sc = *(const f32x4_e*)(bn_scale + c4), bi = *(const f32x4_e*)(bn_bias + c4);
#pragma unroll
                for (int j = 0; j < TP; ++j) {
                    f32x4_e v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float x = fmaxf(__builtin_fmaf(acc[i][j][e], sc[e], bi[e]), 0.f);     // (explicitly fused: the same bits in every instantiation)
                        x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0xB1, 0xF, 0xF, true));    // lane ^ 1
                        x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x4E, 0xF, 0xF, true));    // lane ^ 2
                        x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x141, 0xF, 0xF, true));   // 7 - lane (half row)
                        x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x140, 0xF, 0xF, true));   // 15 - lane (row)
                        v[e] = x * (1.f / 16.f);
                    }
                    int n = cur_n0 + wp * 8 + j;
                    if constexpr (IMAP) n = row_tabs[cur_tsel * 16 + wp * 8 + j];
                    else if (n >= a.N) n = -1;
                    if (l16 == 0 && n >= 0) *(f32x4_e*)(poolp + (size_t)n * oc + chg + wc * 64 + cw) = v;
                }
            }
        } else {
            // straight from the registers: lane (kq, l16) holds, for pixel tile j, channels 8 kq .. + 7 (tiles 0, 1) and 32 + 8 kq .. + 7
            // (tiles 2, 3) of the wave's 64 channels of tile pixel pbase + 16 j + l16; the four lanes of a pixel write 64 contiguous bytes
            const int cw = wc * 64 + 8 * kq;
            f32x4_e sc[4], bi[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                sc[i] = *(const f32x4_e*)(bn_scale + chl + cw + 32 * (i >> 1) + 4 * (i & 1));
                bi[i] = *(const f32x4_e*)(bn_bias + chl + cw + 32 * (i >> 1) + 4 * (i & 1));
            }
#pragma unroll
            for (int j = 0; j < TP; ++j) {
                const int p = pbase + 16 * j + l16;
                // (pad-skip: lane l16 of tile j is image l16 at the tile's position)
                int n = cur_n0 + (SKIP ? l16 : G::p_img(p));
                const int opos = SKIP ? S2Skip::t_y(j) * TW + S2Skip::t_x(wp, j) : G::p_oy(p) * TW + G::p_ox(p);
                if constexpr (IMAP) n = row_tabs[cur_tsel * 16 + G::p_img(p)];      // tensor row, -1 beyond N
                else if (n >= a.N) n = -1;
                _Float16* const dst = outp + ((size_t)(n < 0 ? 0 : n) * (TW * TW) + opos) * oc + chg + cw;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    half8_e o;
#pragma unroll
                    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            float v = acc[2 * h + ii][j][e] * sc[2 * h + ii][e] + bi[2 * h + ii][e];
                            if (a.relu) v = fmaxf(v, 0.f);
                            o[4 * ii + e] = a16_from_f32<BF>(v);
                        }
                    if (n >= 0) *(half8_e*)(dst + 32 * h) = o;
                }
            }
            if constexpr (SKIP) {
                // mixed pair: the other channel group of this workgroup pools through LDS — s_barrier is workgroup-wide: its six barriers
                const float* const pool_o = (a.wgt_b && cur_ch0 + 128 * (1 - g) >= split) ? a.pool_b : a.pool;
                if (pool_o) {
#pragma unroll
                    for (int b = 0; b < 6; ++b) lds_barrier();
                }
            }
        }
        if constexpr (SKIP) pooled_prev = pooled_now;
        stores16 = cur_n0 + IMGS <= a.N;              // (a pooled half issues 32 stores: vmcnt(16) then waits for half of them, never for less)
        vb = nvb;
    }
#undef S2_CHUNKS_S
#undef S2_STEP_S
#undef S2_STEP
#undef END_OF_STEP_WAIT
#undef WAIT_VM
#undef RAW_BARRIER
#undef SETUP_TILE
#undef MASK_DUE
#undef MASK_P
#undef MASK_STORE
#undef MASK_LOAD
#undef ISSUE_P
#undef ISSUE_W
#undef A_TILE
}

template <int TW, bool BF, bool IMAP, bool MSK = false, int CT_ = 256>
__global__ __launch_bounds__(512, 1) void conv3x3_s2_kernel(ConvArgs a, int n_tiles) {
    conv3x3_s2_body<TW, BF, IMAP, MSK, CT_, false>(a, n_tiles);
}

// the pad-skip form of the 8x8 -> 4x4 class ("s2_pad_skip")
template <bool BF>
__global__ __launch_bounds__(512, 1) void conv3x3_s2_skip_kernel(ConvArgs a, int n_tiles) {
    conv3x3_s2_body<4, BF, false, false, 256, true>(a, n_tiles);
}


// Shapes this kernel takes: 3x3 / stride 2 / pad 1, 32x32 -> 16x16, 16x16 -> 8x8 or 8x8 -> 4x4, Cout % 256 == 0 (both convs of
// a pair together), BN + ReLU epilogue.
bool conv_takes_s2_kernel(int ksize, int stride, int pad, int cin, int cout, int h, int w, int ho, int wo) {
    // (Cout % 256 != 0: the 128-channel tiles of the 16x16 output maps)
    return ksize == 3 && stride == 2 && pad == 1 && cin % 32 == 0 && (cout % 256 == 0 || (cout % 128 == 0 && ho == 16)) &&
           cout <= (ho == 4 ? 1024 : 512) && ho == wo && (ho == 16 || ho == 8 || ho == 4) && h == 2 * ho && w == 2 * wo;
}

template <int TW>
static int launch_s2(const ConvArgs& a, int n_cu, hipStream_t s) {
    using G = S2Geom<TW>;
    const bool half = a.Cout % 256 != 0;      // 128-channel tiles (TW == 16)
    const long tiles = (long)((a.N + G::IMGS - 1) / G::IMGS) * (a.Cout / (half ? 128 : 256));
    if (tiles <= 0 || tiles > 0x7fffffffL) return BMI_ERR_INVALID;
    const dim3 grid((unsigned)(tiles < n_cu ? tiles : n_cu)), block(512);
    if (half) {
        if constexpr (TW == 16) {
            if (a.wgt_b || (a.imap && a.in_bits)) return BMI_ERR_UNSUPPORTED;
            ConvArgs al = a;
            al.lazy_order = a.in_bits && opt_lazy_order() && a.in_mod < a.N && a.N % a.in_mod == 0;
            if (a.imap) {      // dynamic early exit: the same kernel family as the full run (the same bits for the images that go on)
                if (a.bf16) hipLaunchKernelGGL((conv3x3_s2_kernel<16, true, true, false, 128>), grid, block, 0, s, al, (int)tiles);
                else hipLaunchKernelGGL((conv3x3_s2_kernel<16, false, true, false, 128>), grid, block, 0, s, al, (int)tiles);
            } else if (a.in_bits) {
                if (a.bf16) hipLaunchKernelGGL((conv3x3_s2_kernel<16, true, false, true, 128>), grid, block, 0, s, al, (int)tiles);
                else hipLaunchKernelGGL((conv3x3_s2_kernel<16, false, false, true, 128>), grid, block, 0, s, al, (int)tiles);
            } else {
                if (a.bf16) hipLaunchKernelGGL((conv3x3_s2_kernel<16, true, false, false, 128>), grid, block, 0, s, al, (int)tiles);
                else hipLaunchKernelGGL((conv3x3_s2_kernel<16, false, false, false, 128>), grid, block, 0, s, al, (int)tiles);
            }
            BMI_CHECK_LAUNCH();
            return BMI_OK;
        } else {
            return BMI_ERR_UNSUPPORTED;
        }
    }
#define S2_LAUNCH(BF_, IMAP_) hipLaunchKernelGGL((conv3x3_s2_kernel<TW, BF_, IMAP_>), grid, block, 0, s, a, (int)tiles)
    if constexpr (TW == 4) {
        // pad-skip form ("s2_pad_skip"): by shape and options only, never by N; row-table launches keep the 4 x 4-block tiles
        if (opt_s2_pad_skip() && !a.imap && !a.in_bits) {
            if (a.bf16) hipLaunchKernelGGL((conv3x3_s2_skip_kernel<true>), grid, block, 0, s, a, (int)tiles);
            else hipLaunchKernelGGL((conv3x3_s2_skip_kernel<false>), grid, block, 0, s, a, (int)tiles);
            BMI_CHECK_LAUNCH();
            return BMI_OK;
        }
    }
    if (a.in_bits) {
        if constexpr (TW == 16) {
            ConvArgs al = a;
            al.lazy_order = opt_lazy_order() && a.in_mod < a.N && a.N % a.in_mod == 0;
            if (a.bf16) hipLaunchKernelGGL((conv3x3_s2_kernel<16, true, false, true>), grid, block, 0, s, al, (int)tiles);
            else hipLaunchKernelGGL((conv3x3_s2_kernel<16, false, false, true>), grid, block, 0, s, al, (int)tiles);
        } else {
            return BMI_ERR_UNSUPPORTED;
        }
    }
    else if (a.imap) { if (a.bf16) S2_LAUNCH(true, true); else S2_LAUNCH(false, true); }
    else { if (a.bf16) S2_LAUNCH(true, false); else S2_LAUNCH(false, false); }
#undef S2_LAUNCH
    BMI_CHECK_LAUNCH();
    return BMI_OK;
}

// BMI_ERR_UNSUPPORTED -> the caller goes on to conv_igemm_wide / conv_igemm.  The minimum-grid rule looks at the engine's
// FULL-CHUNK image count (ConvArgs::n_ref), never at the samples of this launch, like conv3x3_pw's: a t-shard runs the same
// kernel as the single-rank run and gets the same bits ("conv_s2" = 2 drops the rule: tests).
int launch_conv3x3_s2(const ConvArgs& a_in, hipStream_t s) {
    if (!opt_conv_s2() || a_in.in2 || a_in.partial || !conv_epilogue_is_plain(a_in)) return BMI_ERR_UNSUPPORTED;
    // keep bits on the input (ConvArgs::in_bits): the 32x32 -> 16x16 class (one image per tile), a deterministic, pre-scaled input
    if (a_in.in_bits && (a_in.Ho != 16 || a_in.imap || a_in.out_mul != 1.f || a_in.Cin % 32 != 0)) return BMI_ERR_UNSUPPORTED;
    if (a_in.lazy_planar && (!a_in.in_bits || (a_in.W & 1))) return BMI_ERR_UNSUPPORTED;
    if (!conv_takes_s2_kernel(a_in.ksize, a_in.stride, a_in.pad, a_in.Cin, a_in.Cout, a_in.H, a_in.W, a_in.Ho, a_in.Wo)) return BMI_ERR_UNSUPPORTED;
    ConvArgs a = a_in;
    if (a.N <= 0 || a.in_mod <= 0 || a.B <= 0) return BMI_ERR_INVALID;
    if (a.wgt_b && (!a.out_b || a.split <= 0 || a.split >= a.Cout || a.split % 128 != 0)) return BMI_ERR_INVALID;
    if ((a.pool || a.pool_b) && a.Ho != 4) return BMI_ERR_UNSUPPORTED;      // the pooled epilogue sums the 16 lanes of a DPP row = a 4x4 map
    // 32-bit byte offsets inside a buffer descriptor: a tile's own images (always), the whole tensor for the dynamic-exit form
    if (a.imap && (size_t)a.in_mod * a.H * a.W * a.Cin >= 0x7fffffffull) return BMI_ERR_UNSUPPORTED;
    if (a.in_mod < a.N && !a.imap && a.Ho != 16) return BMI_ERR_UNSUPPORTED;      // (tiles of several images take consecutive tensor rows)
    if ((size_t)a.H * a.W * a.Cin >= (1u << 24)) return BMI_ERR_UNSUPPORTED;
    static const int n_cu = [] {
        int dev = 0, cu = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cu = 0;
        return cu > 0 ? cu : 256;
    }();
    if (opt_conv_s2() != 2) {
        const int imgs = 256 / (a.Ho * a.Wo), n_sel = a.n_ref > 0 ? a.n_ref : a.N;
        if ((long)((n_sel + imgs - 1) / imgs) * (a.Cout / (a.Cout % 256 ? 128 : 256)) < 3 * n_cu / 4) return BMI_ERR_UNSUPPORTED;
    }
    a.xcd_split = xcd_split_for(a.Cout / (a.Cout % 256 ? 128 : 256), (size_t)a.Cout * 9 * a.Cin * 2);
    return a.Ho == 16 ? launch_s2<16>(a, n_cu, s) : (a.Ho == 8 ? launch_s2<8>(a, n_cu, s) : launch_s2<4>(a, n_cu, s));
}
