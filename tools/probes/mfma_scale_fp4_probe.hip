// Operand layout of v_mfma_scale_f32_16x16x128_f8f6f4 with FP4 (e2m1) on the A input (cbsz 4) and e4m3 on the B input (blgp 0):
//   1. which k each nibble of an A lane's four registers is, and whether the low nibble is the lower k;
//   2. which lane group's scale byte covers which nibbles on the FP4 side (and which bytes on the e4m3 side, next to FP4).
// Exact integer data only.  k is named by the e4m3 side's layout, which mfma_scale_probe.hip and gemm_fp8.hip's header fix: lane
// (i, g) holds k = 16 g + j in byte j < 16 and k = 64 + 16 g + (j - 16) in byte j >= 16 of its eight registers.
//   1: one A nibble position (lane group ga, nibble ja of the lane's 32) is 1.0 in all 16 rows, one B byte position (gb, jb) is 1.0 in
//      all 16 rows, everything else 0: the output is 1 iff the two positions are the same k.  128 x 128 pairs, one wave per ga/ja.
//   2: all of B is 1.0 and one register (8 nibbles) of one lane group of A is 1.0: every output is 8; then the scale byte of ONE lane
//      group gs is raised to 128: the outputs double iff that group's scale covers those nibbles.  Likewise for the B side.
// hipcc --offload-arch=gfx950 -O2 mfma_scale_fp4_probe.hip -o mfma_scale_fp4_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <cmath>
typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

__device__ __forceinline__ float mfma4(i32x8 a, i32x8 b, int sa, int sb) {
  f32x4 acc = {0, 0, 0, 0};
  acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, acc, /*cbsz: A is fp4*/ 4, /*blgp: B is e4m3*/ 0, 0, sa, 0, sb);
  return fmaxf(fmaxf(acc[0], acc[1]), fmaxf(acc[2], acc[3]));
}

// out[(pa * 128 + pb) * 64 + lane], pa = 32 ga + ja (block), pb = 32 gb + jb.  EVERY lane stores its value: a store from one lane
// alone lets the compiler sink the MFMA into that lane's branch, where it runs with one lane enabled
__global__ void __launch_bounds__(64) pair_kernel(float* out) {
  const int l = threadIdx.x, pa = blockIdx.x, ga = pa >> 5, ja = pa & 31;
  i32x8 a = {0, 0, 0, 0, 0, 0, 0, 0};
  if ((l >> 4) == ga) {
    const int w = 0x2 << (4 * (ja & 7));            // e2m1 1.0 = 0b0010
#pragma unroll
    for (int r = 0; r < 4; ++r) a[r] = (ja >> 3) == r ? w : 0;
  }
  for (int pb = 0; pb < 128; ++pb) {
    const int gb = pb >> 5, jb = pb & 31;
    i32x8 b = {0, 0, 0, 0, 0, 0, 0, 0};
    if ((l >> 4) == gb) {
      const int w = 0x38 << (8 * (jb & 3));         // e4m3 1.0
#pragma unroll
      for (int r = 0; r < 8; ++r) b[r] = (jb >> 2) == r ? w : 0;
    }
    const float v = mfma4(a, b, 127, 127);
    out[(pa * 128 + pb) * 64 + l] = v;
  }
}

// block = ((side * 4 + gd) * 4 + piece) * 4 + gs.  side 0: A sparse (piece = register 0..3: 8 nibbles), side 1: B sparse (piece =
// two registers: 8 bytes, 0..3)
__global__ void __launch_bounds__(64) scale_kernel(float* out) {
  const int l = threadIdx.x, gs = blockIdx.x & 3, piece = (blockIdx.x >> 2) & 3, gd = (blockIdx.x >> 4) & 3, side = blockIdx.x >> 6;
  i32x8 a = {0, 0, 0, 0, 0, 0, 0, 0}, b = {0, 0, 0, 0, 0, 0, 0, 0};
  if (side == 0) {
#pragma unroll
    for (int r = 0; r < 8; ++r) b[r] = 0x38383838;
    if ((l >> 4) == gd) {
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] = piece == r ? 0x22222222 : 0;
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) a[r] = 0x22222222;
    if ((l >> 4) == gd) {
#pragma unroll
      for (int r = 0; r < 8; ++r) b[r] = (r >> 1) == piece ? 0x38383838 : 0;
    }
  }
  const int up = (l >> 4) == gs ? 128 : 127;
  const float v = mfma4(a, b, side == 0 ? up : 127, side == 1 ? up : 127);
  out[blockIdx.x * 64 + l] = v;
}

static int k_of_b(int pb) { const int g = pb >> 5, j = pb & 31; return j < 16 ? 16 * g + j : 64 + 16 * g + (j - 16); }

int main() {
  float *d1, *d2;
  static float h1[128 * 128 * 64], h2[128 * 64];
  CHECK(hipMalloc(&d1, sizeof h1)); CHECK(hipMalloc(&d2, sizeof h2));
  CHECK(hipMemset(d1, 0xff, sizeof h1)); CHECK(hipMemset(d2, 0xff, sizeof h2));
  hipLaunchKernelGGL(pair_kernel, dim3(128), dim3(64), 0, 0, d1);
  hipLaunchKernelGGL(scale_kernel, dim3(128), dim3(64), 0, 0, d2);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(h1, d1, sizeof h1, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(h2, d2, sizeof h2, hipMemcpyDeviceToHost));

  printf("1. k of A nibble (lane group g, register r, nibble n: bits 4n..4n+3), k named by the e4m3 side's layout\n");
  int bad = 0, contiguous = 1;
  for (int pa = 0; pa < 128; ++pa) {
    int hits = 0, k = -1;
    for (int pb = 0; pb < 128; ++pb) {
      float v = 0.f;
      for (int l = 0; l < 64; ++l) v = fmaxf(v, h1[(pa * 128 + pb) * 64 + l]);
      if (v == 1.f) { ++hits; k = k_of_b(pb); } else if (v != 0.f) ++bad;
    }
    if (hits != 1) { ++bad; k = -1; }
    if (k != pa) contiguous = 0;
    if ((pa & 7) == 0) printf("  g %d r %d:", pa >> 5, (pa >> 3) & 3);
    printf(" %3d", k);
    if ((pa & 7) == 7) printf("\n");
  }
  printf("  unexpected outputs: %d\n", bad);
  printf("  lane group g holds k = 32 g + 8 r + n, low nibble = lower k: %s\n", contiguous ? "YES" : "NO");

  for (int side = 0; side < 2; ++side) {
    printf("2%c. %s side: rows = (data lane group, %s), columns = lane group whose scale byte is 128; entry = output / 8\n",
           side ? 'b' : 'a', side ? "e4m3 (B)" : "fp4 (A)", side ? "8-byte piece" : "register");
    for (int gd = 0; gd < 4; ++gd)
      for (int piece = 0; piece < 4; ++piece) {
        printf("  group %d piece %d:", gd, piece);
        for (int gs = 0; gs < 4; ++gs) {
          float v = 0.f;
          for (int l = 0; l < 64; ++l) v = fmaxf(v, h2[(((side * 4 + gd) * 4 + piece) * 4 + gs) * 64 + l]);
          printf(" %4.1f", v / 8);
        }
        printf("\n");
      }
  }
  (void)hipFree(d1); (void)hipFree(d2);
  return bad ? 2 : 0;
}
