/* verify_div_cpu.c -- the check of k_verify_div (mcray-tracing_amd/csrc/mcrt_scene.hip) on the CPU: for every one of the 2^32 float bit
 * patterns x inside the gate of div_res() (1e-18 < |x| < 1e18, or x == 0), does the reciprocal multiply with Markstein's correction
 *
 *     q0 = x * rcp;  r = fmaf(-q0, res, x);  q = fmaf(r, rcp, q0);        rcp = 1.0f / res
 *
 * equal the IEEE quotient x / res AS A VALUE (-0 == +0; a NaN on either side is a mismatch)?  Prints the number of mismatches per texel
 * size: 0 means the GPU may switch its fast voxel quotient on for that tex_res (FrameArgs::fast_div), anything else that it must not.
 * tests/test_gpu_constants.py holds the GPU's verdict against this table.
 *
 * Build and run (host code; -mfma makes fmaf one instruction, -ffp-contract=off keeps the compiler from fusing anything else):
 *
 *     cc -O2 -std=c99 -ffp-contract=off -mfma -fopenmp -o verify_div_cpu tools/verify_div_cpu.c -lm
 *     ./verify_div_cpu                      # the table below: 13 texel sizes, about 15 s each on one core
 *     ./verify_div_cpu 0.145 2e-8           # texel sizes of your own (parsed by strtof)
 *
 * Mismatches (this program, x86-64):
 *     0.145 0.1 0.2 0.25 0.3 0.5 1.0 1/3 2e-8 1e-7 1e-20 1e25     0
 *     3e-30                                                       500518838   (x * rcp overflows from |x| ~ 1e9 on)
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static unsigned long long mismatches(float res)
{
    const float rcp = 1.0f / res;
    unsigned long long bad = 0;
    long long b;
#ifdef _OPENMP
#pragma omp parallel for reduction(+ : bad) schedule(static)
#endif
    for (b = 0; b < (1ll << 32); b++) {
        const uint32_t u = (uint32_t)b;
        float x;
        memcpy(&x, &u, 4);
        const float ax = fabsf(x);
        if (!((ax > 1e-18f && ax < 1e18f) || x == 0.0f)) continue;      /* div_res()'s gate */
        const float q0 = x * rcp;
        const float r = fmaf(-q0, res, x);
        const float q = fmaf(r, rcp, q0);
        if (!(q == x / res)) bad++;
    }
    return bad;
}

int main(int argc, char **argv)
{
    static const char *table[] = { "0.145", "0.1", "0.2", "0.25", "0.3", "0.5", "1.0", "1/3", "2e-8", "1e-7", "1e-20", "1e25", "3e-30" };
    const int n = argc > 1 ? argc - 1 : (int)(sizeof table / sizeof table[0]);
    int k;
    for (k = 0; k < n; k++) {
        const char *s = argc > 1 ? argv[k + 1] : table[k];
        const float res = strcmp(s, "1/3") == 0 ? 1.0f / 3.0f : strtof(s, NULL);
        if (!(res > 0.0f)) { fprintf(stderr, "%s: not a positive float\n", s); return 2; }
        printf("tex_res %-8s = %-14a mismatches %llu\n", s, (double)res, mismatches(res));
        fflush(stdout);
    }
    return 0;
}
