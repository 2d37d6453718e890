// tables.hpp -- layout of the handle's device tables of one-word boards
// (oth_env::tables, written once by k_fill_rays at oth_create), shared by the
// host side (launch.hpp) and the kernels that read them:
//   [0, UP_RAY_WORDS)        rays[d * 64 + sq], d = 0..3 (E, S, SE, SW): the squares
//                            strictly beyond sq toward higher squares (fill_rays);
//                            staged in LDS by the large single-ply launches (RAYS_HALF)
//   [UP_RAY_WORDS, SEL8_AT)  unused (the sel8 table stays where
//                            k_play_rand's and k_playouts' measured code loads it)
//   [SEL8_AT, TABLE_WORDS)   the sel8 table (sel8_word), copied into LDS by
//                            k_play_rand and k_playouts
#pragma once

namespace oth {

constexpr int UP_RAY_WORDS = 4 * 64, SEL8_WORDS = 256;
constexpr int SEL8_AT = 8 * 64, TABLE_WORDS = SEL8_AT + SEL8_WORDS;

}  // namespace oth
