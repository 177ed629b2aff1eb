// K1's tile pass, a group of tiles a wave (streams of large frames within a
// small window): the three grouped fs_tile instances of window 256 and
// their launch.
#include "zk_frame_tile.h"

namespace zk {

int group256_launch(const TileLaunch& l, hipStream_t st) {
  return fs_group_launch<256>(l, st);
}

}  // namespace zk
