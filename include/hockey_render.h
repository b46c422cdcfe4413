/* hockey_render.h -- C ABI of libhockey_render.so: arenas drawn on the GPU (csrc/hk_render.hip, the coverage law
 * of csrc/hk_render.h: hockey/hockey_env.py:697-744 render("rgb_array") as a written per-pixel rule).
 *
 * The renderer reads raw states in hk_get_state's layout (include/hockey.h: [n,18] f32, per body x, y, angle, vx,
 * vy, omega for player 1, player 2 and the puck), not a simulation context: live arenas and logged trajectories
 * draw alike.  Calls are asynchronous on `stream`.  Returns HKR_OK or an error code; hkr_last_error() describes the
 * last failure of the calling thread. */
#ifndef HOCKEY_RENDER_H
#define HOCKEY_RENDER_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HKR_OK 0
#define HKR_E_INVALID 1
#define HKR_E_DEVICE 2

#define HKR_RGB 0   /* out [m, height, width, 3] u8 */
#define HKR_INDEX 1 /* out [m, height, width] u8: palette index 0 white, 1 grey, 2 goal orange, 3 black,
                       4 player 1, 5 player 2 */
#define HKR_STATIC_ONLY 1 /* flags: the rink alone (shapes 1-11), no rackets or puck */

#define HKR_NATIVE_HEIGHT 480
#define HKR_NATIVE_WIDTH 600
#define HKR_MIN_SIZE 4
#define HKR_MAX_SIZE 4096
#define HKR_PALETTE_SIZE 6
#define HKR_CACHED_SIZES 8

const char *hkr_last_error(void);

/* rgb[HKR_PALETTE_SIZE * 3]: the colour of every palette index (host memory; no GPU needed). */
void hkr_palette(uint8_t *rgb);

/* Draw m frames: frame f shows row idx[f] of state (row f when idx is NULL, which needs m <= n_states).
 * state: device [n_states, 18] f32; idx: device [m] i32 or NULL; out: device, 4-byte aligned, layout by `format`;
 * bad_index_count: device counter or NULL.  An idx entry outside [0, n_states) leaves its frame's bytes untouched
 * and adds one to *bad_index_count.  m == 0 is a no-op.
 * HKR_E_INVALID: width % 4 != 0, height or width outside [HKR_MIN_SIZE, HKR_MAX_SIZE], null state / out, a
 * misaligned out, an unknown format or flag, negative counts.
 *
 * The rink (shapes 1-11) is drawn once per (device, height, width) into a palette-index background that later calls
 * read; HKR_CACHED_SIZES sizes are kept per process, the least recently used one is dropped for a new size (the
 * device is synchronised first).  The first call at a size allocates and waits for that background, so it cannot be
 * stream-captured (HKR_E_INVALID); every later call at that size only launches, and is graph-capturable.  A graph
 * captured at a size is valid until that size is dropped or hkr_release() is called. */
int hkr_render(const float *state, int64_t n_states, const int32_t *idx, int64_t m, int32_t height, int32_t width,
               int32_t format, int32_t flags, uint8_t *out, int64_t *bad_index_count, void *stream);

/* Free every cached background (synchronises their devices). */
void hkr_release(void);

#ifdef __cplusplus
}
#endif
#endif
