// tools/palette_host_check.cpp -- TEST INFRASTRUCTURE: one picture through the writer's HOST route with the palette options, in a process
// of its own so that it can be built with -fsanitize=address,undefined (tests/test_writer_palette.py links it against fuif_amd/csrc/*).
//   palette_host_check planes.i32 w h channels bit_depth palette_colors compact_post compact_pre out.fuif
// planes.i32: channels * h * w little-endian int32 samples.  Single-leaf trees (`fuif -I 0`), every pixel loop on the host.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fuifgpu.h"

int main(int argc, char **argv) {
    if (argc != 10) { fprintf(stderr, "usage: %s planes.i32 w h channels bit_depth palette_colors compact_post compact_pre out.fuif\n", argv[0]); return 2; }
    const int w = atoi(argv[2]), h = atoi(argv[3]), nch = atoi(argv[4]), bit_depth = atoi(argv[5]);
    if (w < 1 || h < 1 || nch < 1 || nch > 8) return 2;
    std::vector<int32_t> planes((size_t)w * h * nch);
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(planes.data(), sizeof(int32_t), planes.size(), f) != planes.size()) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    fclose(f);
    fuifgpu_encode_options opt = {sizeof(fuifgpu_encode_options), 1, 1, 12, 0, 4095, 0, 0, 0, 0};
    fuifgpu_palette_options pal = {sizeof(fuifgpu_palette_options), atoi(argv[6]), (float)atof(argv[7]), (float)atof(argv[8])};
    uint8_t *blob = nullptr;
    size_t size = 0;
    const int rc = fuifgpu_encode_image_ex(planes.data(), w, h, nch, bit_depth, &opt, nullptr, &pal, &blob, &size);
    if (rc != FUIFGPU_OK) { fprintf(stderr, "fuifgpu_encode_image_ex: %d (%s)\n", rc, fuifgpu_last_error()); return 1; }
    f = fopen(argv[9], "wb");
    if (!f || fwrite(blob, 1, size, f) != size) { fprintf(stderr, "cannot write %s\n", argv[9]); return 2; }
    fclose(f);
    fuifgpu_free_blob(blob);
    return 0;
}
