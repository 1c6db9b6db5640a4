// gcn10_inflate_internal.hpp -- shared by the two input decoders of libgcn10_gpu.so:
//   gcn10_inflate.hip     inflate_kernel (zlib streams and the status of raw tiles), untile_kernel (the window copy of
//                         every tile that was not decoded in place) and gcn10_gpu_inflate_tiles, which launches all three
//   gcn10_lzw_decode.hip  lzw_decode_kernel (TIFF LZW streams), launched from there between the two
// The device side of a gcn10_inflate_tile (include/gcn10_gpu.h has the caller's side), stated once for the three kernels.
// Each is launched with one workgroup (untile_kernel: one grid column) per tile of the call and picks its tiles by
// their flags.
//
// Flags.  0 = a zlib stream.  GCN10_TILE_RAW = the chunk's bytes lie among the staged bytes as they are.
// GCN10_TILE_LZW = a TIFF LZW stream.  GCN10_TILE_PREDICTOR2 goes with each of the three and concerns untile_kernel alone.
// RAW | LZW names no tile.
//
// Status.  status[tile] is written by exactly one kernel, once:
//   inflate_kernel     every tile without LZW.  A zlib tile: 0, the GCN10_INFLATE_E_* of the first thing wrong with its
//                      stream, or E_WINDOW after a sound stream.  A raw tile: 0, or E_WINDOW if in_len < out_len or the
//                      window does not lie in the chunk (nothing is decoded; no slot, so no slot bound).
//   lzw_decode_kernel  every tile with LZW.  RAW | LZW: E_HEADER.  A window that is refused: E_WINDOW, nothing decoded.
//                      Otherwise 0 or E_LZW_*.
//   untile_kernel      none.  It works out again which tiles the other two have refused (RAW | LZW, inflate_window_ok,
//                      a short raw chunk) and leaves their pixels alone; a tile whose STREAM was bad is copied as far as
//                      it was decoded, zeros behind.
//
// Slot.  Tile i decodes into scratch + i * slot_bytes (slot_bytes = the call's chunk_bytes rounded up to 256, so slots
// are 16-byte aligned) -- except the zlib tiles inflate_kernel decodes straight into the destination (tile_in_place in
// gcn10_inflate.hip; untile_kernel leaves exactly those alone) and raw tiles, which untile_kernel reads where they lie.
//
// Wanted bytes.  min(out_len, slot_bytes): a stream that goes on is cut there.  (out_len > slot_bytes is refused by
// inflate_window_ok unless the window is empty.)
//
// Short streams.  A stream that ends, or fails, before the wanted bytes leaves zeros from there to the wanted bytes'
// end, as the host reader (tiff_codec.c) does.
#ifndef GCN10_INFLATE_INTERNAL_HPP
#define GCN10_INFLATE_INTERNAL_HPP

#include <hip/hip_runtime.h>

#include <cstdint>

#include "gcn10_gpu.h"

namespace gcn10 {

// the window of a gcn10_inflate_tile lies inside its chunk, and the chunk inside a slot of slot_bytes
__device__ __forceinline__ bool inflate_window_ok(uint32_t out_len, uint32_t chunk_w, uint32_t src_x, uint32_t src_y,
                                                  uint32_t copy_w, uint32_t copy_h, uint32_t slot_bytes)
{
    if (copy_w == 0 || copy_h == 0)
        return true;
    if (chunk_w == 0 || out_len > slot_bytes || src_x > chunk_w || copy_w > chunk_w - src_x)
        return false;
    const unsigned long long last = (unsigned long long)(src_y + copy_h - 1u) * chunk_w + src_x + copy_w;
    return (unsigned long long)src_y + copy_h <= 0xffffffffull && last <= out_len;
}

// gcn10_lzw_decode.hip: the GCN10_TILE_LZW tiles of a gcn10_gpu_inflate_tiles call into their slots
void launch_lzw_decode(const uint8_t *comp_dev, const gcn10_inflate_tile *tiles_dev, uint32_t n_tiles,
                       uint8_t *scratch, uint32_t slot_bytes, uint32_t *status_dev, hipStream_t stream);

}  // namespace gcn10

#endif
