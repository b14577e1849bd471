// replica_fork_step.h — the index rules of pu_replica_fork (replica_fork.hip),
// written once: how a replica's bytes are cut into tiles, which bytes of a tile
// a lane moves, and which destinations a workgroup of a group serves.  Plain
// C++ on the host (PU_HD is empty there), __host__ __device__ under hipcc, so
// the stand-alone check (tests/cpp/replica_fork_check.cpp) runs what the kernel
// runs.
//
// A tile is kLanes x kPieces pieces of kPieceBytes: piece u of a tile is one
// contiguous run of kLanes * kPieceBytes = 4 KiB, lane l moving its l-th 16
// bytes, so the lanes of a wave read and write contiguous memory.  A replica is
// a multiple of 4,096 bytes (geometry.cpp: pu::config_geometry), hence of a piece but not
// of a tile: the last tile is masked piece by piece (piece_live).
//
// The destinations [first, first + n) are dealt to G = groups_of(n) groups:
// group g serves first + g, first + g + G, ... and leaves out src.
#pragma once

#include <cstdint>

#include "pu_hd.h"

namespace pu_fork_step {

constexpr int kLanes = 256;
constexpr int kPieces = 4;
constexpr uint64_t kPieceBytes = 16;
constexpr uint64_t kTileBytes = (uint64_t)kLanes * kPieces * kPieceBytes;   // 16 KiB
constexpr int kMaxGroups = 64;

static_assert(kTileBytes == 16384, "a tile is 16 KiB");

PU_HD inline uint64_t tiles_of(uint64_t replica_bytes) { return (replica_bytes + kTileBytes - 1) / kTileBytes; }

// Byte offset within the replica of piece u of `lane` in `tile`.
PU_HD inline uint64_t piece_offset(uint64_t tile, int lane, int u) {
    return tile * kTileBytes + ((uint64_t)u * kLanes + (uint64_t)lane) * kPieceBytes;
}
// replica_bytes is a multiple of kPieceBytes, so a piece that starts inside the replica ends inside it.
PU_HD inline bool piece_live(uint64_t offset, uint64_t replica_bytes) { return offset < replica_bytes; }

PU_HD inline int groups_of(int n) { return n < kMaxGroups ? n : kMaxGroups; }

// Group g's destinations: for (d = dest_begin(first, g); d < dest_end(first, n); d += G) if (dest_taken(d, src)).
PU_HD inline int64_t dest_begin(int first, int g) { return (int64_t)first + g; }
PU_HD inline int64_t dest_end(int first, int n) { return (int64_t)first + n; }
PU_HD inline bool dest_taken(int64_t d, int src) { return d != (int64_t)src; }

// Replicas a fork writes: the range without src.
PU_HD inline int dest_count(int src, int first, int n) { return n - ((src >= first && (int64_t)src < dest_end(first, n)) ? 1 : 0); }

}  // namespace pu_fork_step
