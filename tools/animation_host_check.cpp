// tools/animation_host_check.cpp -- TEST INFRASTRUCTURE: one clip through the writer's HOST route (fuifgpu_encode_animation), in a process
// of its own so that it can be built with -fsanitize=address,undefined (tests/test_writer_animation.py links it against fuif_amd/csrc/*).
//   animation_host_check frames.i32 w frame_h channels frames framerate match_previous palette_colors compact_post compact_pre squeeze out.fuif
// frames.i32: frames * channels * frame_h * w little-endian int32 samples.  8 bits, single-leaf trees (`fuif -I 0`), every loop on the host.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fuifgpu.h"

int main(int argc, char **argv) {
    if (argc != 13) {
        fprintf(stderr, "usage: %s frames.i32 w frame_h channels frames framerate match_previous palette_colors compact_post compact_pre squeeze out.fuif\n", argv[0]);
        return 2;
    }
    const int w = atoi(argv[2]), fh = atoi(argv[3]), nch = atoi(argv[4]), nf = atoi(argv[5]);
    if (w < 1 || fh < 1 || nch < 1 || nch > 8 || nf < 1) return 2;
    std::vector<int32_t> frames((size_t)w * fh * nch * nf);
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(frames.data(), sizeof(int32_t), frames.size(), f) != frames.size()) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    fclose(f);
    fuifgpu_encode_options opt = {sizeof(fuifgpu_encode_options), 1, atoi(argv[11]), 12, 0, 4095, 0, 0, 0, 0};
    fuifgpu_palette_options pal = {sizeof(fuifgpu_palette_options), atoi(argv[8]), (float)atof(argv[9]), (float)atof(argv[10])};
    fuifgpu_animation_options anim = {sizeof(fuifgpu_animation_options), nf, atoi(argv[6]), atoi(argv[7])};
    uint8_t *blob = nullptr;
    size_t size = 0;
    const int rc = fuifgpu_encode_animation(frames.data(), w, fh, nch, 8, &opt, nullptr, &pal, &anim, &blob, &size);
    if (rc != FUIFGPU_OK) { fprintf(stderr, "fuifgpu_encode_animation: %d (%s)\n", rc, fuifgpu_last_error()); return 1; }
    f = fopen(argv[12], "wb");
    if (!f || fwrite(blob, 1, size, f) != size) { fprintf(stderr, "cannot write %s\n", argv[12]); return 2; }
    fclose(f);
    fuifgpu_free_blob(blob);
    return 0;
}
