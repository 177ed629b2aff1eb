// K1's tile pass, one tile a wave: the eight single-tile fs_tile instances
// (four windows, with and without long-frame mode) and their launch.
#include "zk_frame_tile.h"

namespace zk {

int tile_launch(const TileLaunch& l, hipStream_t st) {
  if (l.G != 1) return -1;
  if (l.lng) {
    switch (l.W) {
      case 256: return fs_tile_launch<256, true, 1>(l, st);
      case 512: return fs_tile_launch<512, true, 1>(l, st);
      case 1024: return fs_tile_launch<1024, true, 1>(l, st);
      default: return fs_tile_launch<2048, true, 1>(l, st);
    }
  }
  switch (l.W) {
    case 256: return fs_tile_launch<256, false, 1>(l, st);
    case 512: return fs_tile_launch<512, false, 1>(l, st);
    case 1024: return fs_tile_launch<1024, false, 1>(l, st);
    default: return fs_tile_launch<2048, false, 1>(l, st);
  }
}

}  // namespace zk
