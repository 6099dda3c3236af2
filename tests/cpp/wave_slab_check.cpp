// wave_slab_check — the 8-lane block kernel's per-wave LDS regions and record stores (pba_wave_slab.h), on the host.
//
// photometric_block_kernel gives each of its four waves one LDS region (its 8 tile blocks, then its 8 staged records
// over the same bytes) and lets each wave store its own run of records.  A store past the end of the record array is
// not something a GPU test can see, so the ranges are checked here for every record format × P = 1…8 × live blocks
// 1…32 of a tile, with the functions the kernel itself calls:
//   - the waves' store ranges are disjoint, in order, and together cover exactly nblk records (no byte past them);
//   - a wave's range starts 16-B aligned where the tile's slab does (a tile starts at a multiple of 32 records);
//   - each range is read from inside its wave's LDS region;
//   - the four regions do not overlap, hold 8 tile blocks and 8 records each, and fit the kernel's LDS array.
// The stores are replayed into a guarded buffer (the sanitizers catch an out-of-range write; every byte must be written
// exactly once).  Prints one JSON line; a violated condition or a sanitizer report ends it with a non-zero exit.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pba_wave_slab.h"

using namespace pba::detail;

namespace {

// the formats the kernel is built for: pba_wave_slab.h's table, which pba_record.h ties to RecFormat<T>
using Format = SlabFormat;

long long g_checks = 0;
#define REQUIRE(c)                                                                          \
  do {                                                                                      \
    ++g_checks;                                                                             \
    if (!(c)) {                                                                             \
      std::fprintf(stderr, "wave_slab_check: %s failed (%s:%d) fmt=%s P=%d nblk=%d w=%d\n", \
                   #c, __FILE__, __LINE__, f.name, P, nblk, w);                             \
      std::exit(1);                                                                         \
    }                                                                                       \
  } while (0)

}  // namespace

int main() {
  long long cases = 0, bytes_total = 0;
  for (const Format& f : kSlabFormats) {
    for (int records = 0; records < 2; ++records) {
      int P = 0, nblk = 0, w = 0;
      const int region = wave_region_bytes(f.cols, f.ssize, records != 0);
      const int lds = wg_lds_bytes(f.cols, f.ssize, records != 0);
      REQUIRE(region % 16 == 0);
      REQUIRE(kSlabWaves * region == lds);
      REQUIRE(lds <= 64 * 1024);
      // the regions: wave w's is [w·region, (w+1)·region), so they are disjoint; each holds its 8 tile blocks
      for (int lb = 0; lb < kSlabWaves * kSlabWaveBlocks; ++lb) {
        w = lb / kSlabWaveBlocks;
        const int o = tile_block_offset(lb, region);
        REQUIRE(o % 16 == 0);
        REQUIRE(o == wave_region_offset(w, region) + (lb % kSlabWaveBlocks) * kSlabTileBytes);  // the kernel's form
        REQUIRE(o >= w * region && o + kSlabTileBytes <= (w + 1) * region);
        if (lb % kSlabWaveBlocks) REQUIRE(o == tile_block_offset(lb - 1, region) + kSlabTileBytes);
      }
      if (!records) continue;
      for (P = 1; P <= kSlabMaxPattern; ++P) {
        const int rec_bytes = f.cols * P * f.ssize;
        for (int lb = 0; lb < kSlabWaves * kSlabWaveBlocks; ++lb) {
          w = lb / kSlabWaveBlocks;
          const int o = staged_record_offset(lb, region, rec_bytes);
          REQUIRE(o >= w * region && o + rec_bytes <= (w + 1) * region);
          REQUIRE(o - wave_region_offset(w, region) == (lb % kSlabWaveBlocks) * rec_bytes);  // contiguous from the region's start
        }
        for (nblk = 1; nblk <= kSlabWaves * kSlabWaveBlocks; ++nblk) {
          ++cases;
          // the tile's slab: exactly nblk records, allocated to the byte so that the sanitizer sees a store past it
          std::vector<unsigned char> slab((size_t)nblk * rec_bytes, 0);
          int end = 0;
          for (w = 0; w < kSlabWaves; ++w) {
            const WaveStore s = wave_store_range(w, nblk, rec_bytes);
            REQUIRE(s.bytes >= 0 && s.bytes % rec_bytes == 0);
            REQUIRE(s.bytes <= region);  // read from inside the wave's region
            // a tile's slab starts at record 32·tile: 16-B aligned in a 16-B aligned array; so is every wave's start
            REQUIRE(s.begin % 16 == 0);
            if (s.bytes) {
              REQUIRE(s.begin == end);  // in order, no gap, no overlap
              for (int i = 0; i < s.bytes; ++i) ++slab.data()[s.begin + i];
              end = s.begin + s.bytes;
            }
            // the blocks the wave staged are the blocks it stores
            const int first = w * kSlabWaveBlocks;
            const int live = nblk - first < 0 ? 0 : (nblk - first > kSlabWaveBlocks ? kSlabWaveBlocks : nblk - first);
            REQUIRE(s.bytes == live * rec_bytes);
            if (live) REQUIRE(s.begin == first * rec_bytes);
          }
          w = -1;
          REQUIRE(end == nblk * rec_bytes);
          for (size_t i = 0; i < slab.size(); ++i) REQUIRE(slab[i] == 1);
          bytes_total += end;
        }
      }
    }
  }
  std::printf("{\"formats\": %d, \"cases\": %lld, \"checks\": %lld, \"bytes\": %lld}\n",
              kSlabFormatCount, cases, g_checks, bytes_total);
  return 0;
}
