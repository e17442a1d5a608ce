// bfgx_tile_arena.hpp -- the counter arena of the shell plan (host code only): the ONE device allocation that holds everything a step
// resets, and the one place where its layout is written down.  In 32-bit words from the base:
//
//   cnt_a_pad     ntiles * cnt_pad, rounded up to 4   counters of the tiles' fixed lists entries_a[tile][cap_a] (K0 places the few-tile halos
//                                of a fast plan there itself), cnt_pad words apart (see wave_run_issue)
//   cnt_b         ntiles + 1     entries of every tile in the shared list (K0): what did not fit the fixed list, halos over more than
//                                kRefMax tiles, and every halo of a generic plan
//   cur_b         ntiles + 1     cursors of the placement pass (ensure_entry_capacity resets them for a second pass)
//   tile_counter  1              the counter the persistent K1 / K3 grids draw their tiles from
//   omax          ntiles + 1     largest |offset|^2 of every tile (K1's flush or tile_reach_kernel): the reach of the gathering regrid
//   (rounded up to 4 words)
//   ctrl          8              RegridCtrl: entries of the far list and of its source list, overflow of the full-map regrid, tiles left to
//                                the walking kernel
//   ---- the step's one memset zeroes [base, here): a single buffer and a multiple of 16 bytes (two buffers, or another length, cost a
//        4.5 us fill kernel each) ----
//   todo_list     ntiles         the tiles left to the walking kernel: RegridCtrl.todo_count is the word in front of them, so that
//                                `todo` = {count, tiles ...} is one array to the kernels
//   band_overflow 1              overflow flag of the far list in the banded regrid (an error there; the full-map regrid repairs it)
//   (3 spare words)
//
// The regions are packed: only the two roundings above leave gaps.  ntiles * cnt_pad is a multiple of four for every default tiling
// (cnt_pad is 32, 8 or 2) and the first rounding adds nothing there; the BFGX_TILE_W / BFGX_TILE_BR tilings can reach cnt_pad 1, where
// it is what keeps RegridCtrl's 64-bit counter aligned and the memset a multiple of 16 bytes.
#pragma once
#include <cstddef>
#include <cstdint>

namespace bfgx {

// the regrid's control words, reset together (regrid_impl) and read back together (bfgx_plan_regrid_stats)
struct RegridCtrl {
    unsigned long long far_count;    // FarList.count: entries appended (may exceed the capacity)
    uint32_t far_src_count;          // FarSrc.count: source pixels listed for the generic route (may exceed the capacity); follows far_count: one memset resets both
    int32_t spare[3];                // (the step's memset stays a multiple of 16 bytes)
    int32_t far_overflow_full;       // full-map regrid: overflow of either list is repaired in-stream (pass 1), not an error
    int32_t todo_count;              // tiles the lean gather kernel leaves to the one with the ring walk (followed by their numbers)
};
static_assert(sizeof(RegridCtrl) == 32 && alignof(RegridCtrl) == 8, "RegridCtrl is eight words, the first two a 64-bit counter");
static_assert(offsetof(RegridCtrl, far_src_count) == 8 && offsetof(RegridCtrl, todo_count) == 28, "the two list counters are adjacent; the todo count is the last word");

constexpr size_t kFarCountersBytes = offsetof(RegridCtrl, far_src_count) + sizeof(uint32_t);      // what a banded regrid that starts both lists afresh zeroes
constexpr size_t kCtrlWords =sizeof(RegridCtrl) / sizeof(int32_t);
constexpr size_t round_up4(size_t words) { return (words + 3) & ~(size_t)3; }

// word offsets of the regions from the base, and the lengths the host needs
struct TileArenaLayout {
    size_t cnt_a_pad, cnt_b, cur_b, tile_counter, omax, ctrl, far_overflow_full, todo, todo_list, band_overflow;
    size_t cursor_words;     // cur_b
    size_t zeroed_words;     // the per-step memset: [base, end of ctrl)
    size_t tail_words;       // ctrl and everything behind it (zeroed once, at plan creation)
    size_t total_words;
};

constexpr TileArenaLayout tile_arena_layout(size_t ntiles, size_t cnt_pad)
{
    const size_t blk = ntiles + 1;
    TileArenaLayout L{};
    L.cnt_a_pad = 0;
    L.cnt_b = round_up4(ntiles * cnt_pad);
    L.cur_b = L.cnt_b + blk;
    L.tile_counter = L.cur_b + blk;
    L.omax = L.tile_counter + 1;
    L.ctrl = L.cnt_b + round_up4(L.omax + blk - L.cnt_b);
    L.far_overflow_full = L.ctrl + offsetof(RegridCtrl, far_overflow_full) / sizeof(int32_t);
    L.todo = L.ctrl + offsetof(RegridCtrl, todo_count) / sizeof(int32_t);
    L.todo_list = L.ctrl + kCtrlWords;
    L.band_overflow = L.todo_list + ntiles;
    L.cursor_words = L.tile_counter - L.cur_b;
    L.zeroed_words = L.ctrl + kCtrlWords;
    L.total_words = L.band_overflow + 4;
    L.tail_words = L.total_words - L.ctrl;
    return L;
}

// the arena as the launches see it
struct TileArena {
    int32_t *base = nullptr;           // == cnt_a_pad: what the step's memset starts at
    int32_t *cnt_a_pad = nullptr, *cnt_b = nullptr, *cur_b = nullptr;
    unsigned int *tile_counter = nullptr;
    float *omax = nullptr;
    RegridCtrl *ctrl = nullptr;
    int32_t *far_overflow_full = nullptr;
    int32_t *todo = nullptr;           // [0] = RegridCtrl.todo_count, then the tiles
    int32_t *band_overflow = nullptr;
    size_t cursor_bytes = 0, zeroed_bytes = 0, tail_bytes = 0;

    void bind(int32_t *b, const TileArenaLayout &L)
    {
        base = b;
        cnt_a_pad = b + L.cnt_a_pad; cnt_b = b + L.cnt_b; cur_b = b + L.cur_b;
        tile_counter = (unsigned int *)(b + L.tile_counter);
        omax = (float *)(b + L.omax);
        ctrl = (RegridCtrl *)(b + L.ctrl);
        far_overflow_full = b + L.far_overflow_full;
        todo = b + L.todo;
        band_overflow = b + L.band_overflow;
        cursor_bytes = sizeof(int32_t) * L.cursor_words;
        zeroed_bytes = sizeof(int32_t) * L.zeroed_words;
        tail_bytes = sizeof(int32_t) * L.tail_words;
    }
};

// the scratch of the multi-workgroup tile scan: one total and one offset per scan block (tile_scan_part_kernel, tile_scan_blocks_kernel;
// the launch takes that route up to 1024 blocks)
constexpr size_t kScanBlocksRoom = 1024;
struct ScanScratchLayout { size_t block_tot, block_off, total_words; };
constexpr ScanScratchLayout scan_scratch_layout()
{
    ScanScratchLayout L{};
    L.block_tot = 0;
    L.block_off = L.block_tot + kScanBlocksRoom;
    L.total_words = L.block_off + kScanBlocksRoom;
    return L;
}
struct ScanScratch {
    int32_t *block_tot = nullptr, *block_off = nullptr;
    void bind(int32_t *b, const ScanScratchLayout &L) { block_tot = b + L.block_tot; block_off = b + L.block_off; }
};

// ---- the facts the kernels and the launches rely on, checked where the layout is computed
template <size_t NT, size_t PAD>
struct TileArenaCheck {
    static constexpr TileArenaLayout L = tile_arena_layout(NT, PAD);
    static constexpr size_t blk = NT + 1;
    static constexpr bool unrounded = (NT * PAD) % 4 == 0;
    static constexpr size_t n3p = round_up4(3 * blk + 1);          // the three blocks of ntiles + 1 words and the tile counter, rounded up to four words
    // regions in the documented order, none overlapping the next
    static_assert(L.cnt_a_pad == 0 && L.cnt_b >= NT * PAD, "the padded counters start the arena and hold ntiles * cnt_pad words");
    static_assert(L.cur_b == L.cnt_b + blk && L.cursor_words == blk && L.tile_counter == L.cur_b + L.cursor_words,
                  "cnt_b and cur_b: ntiles + 1 words each, and nothing else lies in the cursors' span");
    static_assert(L.omax == L.tile_counter + 1, "the |offset|^2 block follows the tile counter");
    static_assert(L.ctrl >= L.omax + blk && L.ctrl - (L.omax + blk) < 4, "the control words follow the three blocks and the tile counter, rounded up to four words");
    static_assert(L.far_overflow_full == L.ctrl + 6 && L.todo == L.ctrl + 7 && L.todo_list == L.todo + 1, "count (64 bits), source count, three spare, overflow, todo count, todo tiles");
    static_assert(L.band_overflow == L.todo_list + NT && L.total_words > L.band_overflow, "the banded overflow flag follows the todo tiles, inside the allocation");
    // the step's memset
    static_assert(L.zeroed_words == L.ctrl + kCtrlWords, "the zeroed span starts at the base and ends exactly after RegridCtrl");
    static_assert(L.zeroed_words % 4 == 0, "the zeroed span is a multiple of 16 bytes");
    static_assert(L.todo_list >= L.zeroed_words && L.band_overflow >= L.zeroed_words, "the step's memset touches neither the todo tiles nor the banded overflow flag");
    static_assert(L.ctrl % 2 == 0, "RegridCtrl's 64-bit counter is 8-byte aligned (the base is a device allocation)");
    static_assert(L.tail_words == L.total_words - L.ctrl && L.tail_words == NT + 12, "plan creation zeroes the control words and all behind them");
    // packed: the padded region holds exactly ntiles * cnt_pad words wherever that is a multiple of four, and the lengths follow from it
    static_assert(L.cnt_b == round_up4(NT * PAD) && (!unrounded || L.cnt_b == NT * PAD), "only a padded region that is no multiple of four words is rounded up");
    static_assert(L.tile_counter == L.cnt_b + 2 * blk && L.omax == L.cnt_b + 2 * blk + 1 && L.ctrl == L.cnt_b + n3p, "the three blocks, the tile counter between the second and the third");
    static_assert(L.zeroed_words == L.cnt_b + n3p + 8 && L.total_words == L.cnt_b + n3p + NT + 12, "lengths of the memset and of the allocation");
    static constexpr bool ok = true;
};
// one scan block (NSIDE 1, 2, 8, 16), the benchmark's NSIDE 1024, NSIDE 4096 and 8192 with their narrower padding, and two tilings
// only the BFGX_TILE_W / BFGX_TILE_BR knobs reach: cnt_pad 1 with ntiles = 3 and = 1 (mod 4)
static_assert(TileArenaCheck<1, 32>::ok && TileArenaCheck<2, 32>::ok && TileArenaCheck<14, 32>::ok && TileArenaCheck<52, 32>::ok &&
              TileArenaCheck<6208, 32>::ok && TileArenaCheck<98560, 8>::ok && TileArenaCheck<393728, 2>::ok &&
              TileArenaCheck<3, 1>::ok && TileArenaCheck<12289, 1>::ok, "tile arena layout");

static_assert(scan_scratch_layout().block_tot == 0 && scan_scratch_layout().block_off == 1024 && scan_scratch_layout().total_words == 2048,
              "scan scratch: 1024 totals, then 1024 offsets: one word each per scan block");

}  // namespace bfgx
