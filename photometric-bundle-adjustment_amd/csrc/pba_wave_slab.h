// pba_wave_slab.h — where the 8-lane block kernel (photometric_block_kernel, pba_evaluate.hip) keeps a workgroup's
// 32 blocks in LDS and which bytes of the record array each of its four waves stores.  Plain C++ (no HIP types): the
// kernel and the host check (tests/cpp/wave_slab_check.cpp) read the same functions.
//
// A workgroup is 4 waves of 64 lanes, 8 lanes per block: wave w evaluates blocks 8w … 8w+7 of the tile.  Wave w owns
// one LDS region that holds first those blocks' tile blocks (written by the cooperative prologue, read by the wave's
// rows) and then, over the same bytes, their staged records — so after the prologue's barrier a wave writes only LDS
// bytes that it alone reads, and it stores its own contiguous run of records without waiting for the other waves.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PBA_HD __host__ __device__
#else
#define PBA_HD
#endif

namespace pba {
namespace detail {

constexpr int kSlabWaves = 4;         // waves per workgroup
constexpr int kSlabWaveBlocks = 8;    // blocks per wave
constexpr int kSlabMaxPattern = 8;    // pixels per block of the 8-lane kernel
constexpr int kSlabTileBytes = 352;   // sizeof(TileBlock) (pba_evaluate.hip asserts it)

// The record formats the kernel is built for: columns per pixel row and bytes per stored value, in the order fp32,
// PBA_RECORD_F16, PBA_RECORD_F16_SCALED, free intrinsics, affine brightness, both.  pba_record.h ties every
// RecFormat<T> to its entry and the kernel refuses (static_assert) a format that has none, so the host check, which
// walks this table, sees every format the kernel can be instantiated with.
struct SlabFormat {
  const char* name;
  int cols, ssize;
};
constexpr SlabFormat kSlabFormats[] = {{"f32", 14, 4},  {"f16", 14, 2},    {"scaled", 15, 2},
                                       {"intr", 22, 4}, {"affine", 18, 4}, {"intr_affine", 26, 4}};
constexpr int kSlabFormatCount = (int)(sizeof(kSlabFormats) / sizeof(kSlabFormats[0]));
PBA_HD constexpr bool slab_format_known(int cols, int ssize) {
  for (int i = 0; i < kSlabFormatCount; ++i)
    if (kSlabFormats[i].cols == cols && kSlabFormats[i].ssize == ssize) return true;
  return false;
}

// Bytes of one wave's LDS region for records of `cols` stored values of `ssize` bytes per pixel (records = false: a
// launch that stages no record): its 8 tile blocks or its 8 largest records, whichever is more.  A multiple of 16.
PBA_HD constexpr int wave_region_bytes(int cols, int ssize, bool records = true) {
  const int tile = kSlabWaveBlocks * kSlabTileBytes;
  const int stage = records ? kSlabWaveBlocks * cols * kSlabMaxPattern * ssize : 0;
  return stage > tile ? stage : tile;
}
// The kernel's LDS array: the four regions, wave w's at w · wave_region_bytes.
PBA_HD constexpr int wg_lds_bytes(int cols, int ssize, bool records = true) {
  return kSlabWaves * wave_region_bytes(cols, ssize, records);
}
// LDS byte offset of wave w's region, of tile block lb (0 … 31) and of block lb's staged record of rec_bytes bytes.
PBA_HD constexpr int wave_region_offset(int w, int region) { return w * region; }
PBA_HD constexpr int tile_block_offset(int lb, int region) {
  return wave_region_offset(lb / kSlabWaveBlocks, region) + (lb % kSlabWaveBlocks) * kSlabTileBytes;
}
PBA_HD constexpr int staged_record_offset(int lb, int region, int rec_bytes) {
  return wave_region_offset(lb / kSlabWaveBlocks, region) + (lb % kSlabWaveBlocks) * rec_bytes;
}

// What wave w stores for a tile of nblk live blocks (1 … 32) with records of rec_bytes bytes: `bytes` bytes from LDS
// offset w · region to byte `begin` of the tile's slab (the tile's first record is byte 0).
struct WaveStore {
  int begin, bytes;
};
PBA_HD constexpr WaveStore wave_store_range(int w, int nblk, int rec_bytes) {
  const int first = w * kSlabWaveBlocks;
  const int n = nblk - first < 0 ? 0 : (nblk - first > kSlabWaveBlocks ? kSlabWaveBlocks : nblk - first);
  return {first * rec_bytes, n * rec_bytes};
}

}  // namespace detail
}  // namespace pba
