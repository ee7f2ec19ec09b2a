"""The unsqueeze kernels run a branch-free form of the reference's two Squeeze formulas (fuif_amd/csrc/squeeze_arith.h).
This compiles that header for the host next to the formulas as the reference writes them (transform/squeeze.h:61-77,103-107)
and compares them case by case: every triple of a small cube (all orderings, ties and parities) and tens of millions of random
triples at scales up to 2^21 (samples have at most 17 significant bits).

The reference keeps every sample in pixel_type = int16_t (image/image.h:35), and inv_hsqueeze / inv_vsqueeze declare tendency, diff,
A and B as pixel_type (squeeze.h:98-108): the second half restates that step with int16_t-typed variables and compares it with the
header's unsqueeze_step (what all unsqueeze kernels call) on a dense small cube of quadruples (left, avg, next_avg, residual), on
every combination of the corner values of int16, and on 30 M random quadruples over the full int16 range.  The same cases compare
smooth_tendency itself (int arithmetic, no narrowing inside) with the reference's int16-typed function: for int16 inputs nothing in
it leaves 16 bits, which is why the header narrows only diff, A and B."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include "squeeze_arith.h"
// transform/squeeze.h:61-77 as written there
static int ref_tendency(int B, int a, int n) {
    int diff = 0;
    if (B >= a && a >= n) {
        diff = (4 * B - 3 * n - a + 6) / 12;
        if (diff - (diff & 1) > 2 * (B - a)) diff = 2 * (B - a) + 1;
        if (diff + (diff & 1) > 2 * (a - n)) diff = 2 * (a - n);
    } else if (B <= a && a <= n) {
        diff = (4 * B - 3 * n - a - 6) / 12;
        if (diff + (diff & 1) < 2 * (B - a)) diff = 2 * (B - a) - 1;
        if (diff - (diff & 1) < 2 * (a - n)) diff = 2 * (a - n);
    }
    return diff;
}
// squeeze.h:103-107
static void ref_pair(int avg, int diff, int &A, int &B) { A = ((avg << 1) + diff + (diff > 0 ? -(diff & 1) : (diff & 1))) >> 1; B = A - diff; }
// squeeze.h:61-77 and :98-108 with the reference's types: pixel_type = int16_t (image/image.h:35) for the parameters, the result and every
// local; the arithmetic itself runs in promoted int and each assignment narrows
typedef int16_t pixel_type;
static pixel_type ref16_tendency(pixel_type B, pixel_type a, pixel_type n) {
    pixel_type diff = 0;
    if (B >= a && a >= n) {
        diff = (4 * B - 3 * n - a + 6) / 12;
        if (diff - (diff & 1) > 2 * (B - a)) diff = 2 * (B - a) + 1;
        if (diff + (diff & 1) > 2 * (a - n)) diff = 2 * (a - n);
    } else if (B <= a && a <= n) {
        diff = (4 * B - 3 * n - a - 6) / 12;
        if (diff + (diff & 1) < 2 * (B - a)) diff = 2 * (B - a) - 1;
        if (diff - (diff & 1) < 2 * (a - n)) diff = 2 * (a - n);
    }
    return diff;
}
static void ref16_step(pixel_type left, pixel_type avg, pixel_type next_avg, pixel_type diff_minus_tendency, pixel_type &A, pixel_type &B) {
    pixel_type tendency = ref16_tendency(left, avg, next_avg);
    pixel_type diff = diff_minus_tendency + tendency;
    A = ((avg << 1) + diff + (diff > 0 ? -(diff & 1) : (diff & 1))) >> 1;
    B = A - diff;
}
static long bad16 = 0, n16 = 0;
static void check16(int left, int avg, int next_avg, int res) {
    pixel_type A1, B1;
    ref16_step((pixel_type)left, (pixel_type)avg, (pixel_type)next_avg, (pixel_type)res, A1, B1);
    int A2, B2;
    fuifgpu::unsqueeze_step(left, avg, next_avg, res, A2, B2);
    n16++;
    bad16 += (A2 != (int)A1 || B2 != (int)B1);
    bad16 += fuifgpu::smooth_tendency(left, avg, next_avg) != (int)ref16_tendency((pixel_type)left, (pixel_type)avg, (pixel_type)next_avg);
}
int main() {
    long bad = 0, n = 0;
    for (int B = -40; B <= 40; B++) for (int a = -40; a <= 40; a++) for (int c = -40; c <= 40; c++) { n++; bad += ref_tendency(B, a, c) != fuifgpu::smooth_tendency(B, a, c); }
    unsigned long long x = 88172645463325252ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (unsigned)(x >> 16); };
    for (long i = 0; i < 30000000; i++) {
        const int sc = 1 << (rnd() % 22);
        const int B = (int)(rnd() % (2u * sc + 1)) - sc, a = B + ((int)(rnd() % (2u * sc + 1)) - sc) / (int)(1 + rnd() % 8), c = a + ((int)(rnd() % (2u * sc + 1)) - sc) / (int)(1 + rnd() % 8);
        n++; bad += ref_tendency(B, a, c) != fuifgpu::smooth_tendency(B, a, c);
    }
    for (int avg = -200; avg <= 200; avg++) for (int d = -500; d <= 500; d++) { int A1, B1, A2, B2; ref_pair(avg, d, A1, B1); fuifgpu::unsqueeze_pair(avg, d, A2, B2); n++; bad += (A1 != A2 || B1 != B2); }
    for (long i = 0; i < 10000000; i++) { const int avg = (int)(rnd() % 4000001u) - 2000000, d = (int)(rnd() % 4000001u) - 2000000; int A1, B1, A2, B2; ref_pair(avg, d, A1, B1); fuifgpu::unsqueeze_pair(avg, d, A2, B2); n++; bad += (A1 != A2 || B1 != B2); }
    // the int16 step: a dense cube (all orderings, ties, parities and signs of the residual), ...
    for (int l = -12; l <= 12; l++) for (int a = -12; a <= 12; a++) for (int c = -12; c <= 12; c++) for (int r = -30; r <= 30; r++) check16(l, a, c, r);
    // ... every combination of the corners of int16, ...
    static const int corner[7] = {-32768, -32767, -1, 0, 1, 32766, 32767};
    for (int i = 0; i < 7; i++) for (int j = 0; j < 7; j++) for (int k = 0; k < 7; k++) for (int m = 0; m < 7; m++) check16(corner[i], corner[j], corner[k], corner[m]);
    // ... and random quadruples over the full int16 range: independent ones, and ones whose three samples lie close together (the
    // monotone branches of the tendency, which independent samples enter only a third of the time)
    for (long i = 0; i < 20000000; i++) check16((int)(rnd() & 0xFFFF) - 32768, (int)(rnd() & 0xFFFF) - 32768, (int)(rnd() & 0xFFFF) - 32768, (int)(rnd() & 0xFFFF) - 32768);
    for (long i = 0; i < 12000000; i++) {
        const int sc = 1 << (rnd() % 16);
        const int l = (int)(rnd() & 0xFFFF) - 32768;
        int a = l + (int)(rnd() % (2u * sc + 1)) - sc, c = a + (int)(rnd() % (2u * sc + 1)) - sc;
        a = a < -32768 ? -32768 : (a > 32767 ? 32767 : a);
        c = c < -32768 ? -32768 : (c > 32767 ? 32767 : c);
        check16(l, a, c, (int)(rnd() & 0xFFFF) - 32768);
    }
    printf("%ld cases, %ld mismatches\n", n, bad);
    printf("int16 step: %ld cases, %ld mismatches\n", n16, bad16);
    return bad != 0 || bad16 != 0;
}
"""


def test_branch_free_squeeze_formulas_equal_the_reference_form(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("needs g++")
    src = tmp_path / "harness.cpp"
    src.write_text(HARNESS)
    exe = str(tmp_path / "harness")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "fuif_amd", "csrc"), str(src), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout
    assert "int16 step: " in r.stdout and r.stdout.count(" 0 mismatches") == 2, r.stdout
