// scan_wide_probe.hip -- diagnostic build of scan_wide.hip with per-wave s_memtime accumulators.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o scan_wide_probe scan_wide_probe.hip
//   ./scan_wide_probe <rows> <dim> <nq> <k>
// The 24- / 32-slot forms run as the product launches them: nt stream for slabs of 1 GB and more, ticketed tile schedule on long
// streams (85 % of the tiles in granules of 8; CRS_WIDE_DYN=0: static stride), CRS_WIDE_STAGGER, CRS_WIDE_MFMA and CRS_WIDE_RING as in the
// library.  In the ring kernels (scan_wide.hip, "Ring form") the laps follow the new issue points: "wait next tile" and "tile-load issue"
// lie behind the selection (waves 0-3) resp. between the deferred selection and the MFMA sweep (waves 4-7), and "barrier" is the raw
// barrier at the iteration's end.
// The last line is the clock the chip held inside the kernel: a wave's cycles over the launch / the launch's time.
// Slot 5 is not a lap but a count: how often a wave ran the insertion chain of the deferred split forms (CRS_WIDE_DEFER, scan_wide.hip
// "Deferred insertion"; one more than the flushes in the loop: the flush at the end).  That count depends on the data, so the slab is
// filled on the device with rows that do not repeat.
#define CRS_STAMPS 1
#define CRS_WIDE_TU 2   // the two-buffer kernels and the ring kernels
#include "../compressed-rag-suite_amd/csrc/scan_wide.hip"
#include "../compressed-rag-suite_amd/csrc/plan.cpp"   // knobs_from_env

#include <algorithm>
#include <math.h>
#include <stdio.h>
#include <vector>

// one thread per 8 elements: a sum of four hashed uniforms per element, scaled like the host's queries
__global__ void fill_rows(_Float16* slab, size_t n8, float sc) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;
  for (int e = 0; e < 8; ++e) {
    unsigned long long z = (i * 8 + e) * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    float u = 0;
    for (int j = 0; j < 4; ++j) u += ((z >> (16 * j)) & 0xffff) / 65536.0f - 0.5f;
    slab[i * 8 + e] = (_Float16)(u * sc);
  }
}

int main(int argc, char** argv) {
  const int rows = argc > 1 ? atoi(argv[1]) : 1250000;
  const int dim = argc > 2 ? atoi(argv[2]) : 384;
  const int nq = argc > 3 ? atoi(argv[3]) : 256;
  const int k = argc > 4 ? atoi(argv[4]) : 10;
  const crs::Knobs kn = crs::knobs_from_env();
  const int nw = (nq > 64 && crs::wide_serves(k, dim)) ? (nq > 128 ? 8 : 4) : 0;
  if (!nw) { printf("wide kernel not applicable\n"); return 1; }
  const int tile_rows = crs::scan_wide_tile_rows(nw, dim);
  const int n_tiles = (rows + tile_rows - 1) / tile_rows;
  hipDeviceProp_t prop; hipGetDeviceProperties(&prop, 0);
  const int nqb = (nq + 32 * nw - 1) / (32 * nw);
  int nwg = prop.multiProcessorCount * crs::scan_wide_wg_per_cu(nw) / nqb;
  if (nqb > 1) nwg &= ~7;
  nwg = std::min(nwg, n_tiles);
  std::vector<_Float16> hq((size_t)nq * dim);
  unsigned s = 12345;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; float u = 0; for (int i = 0; i < 4; ++i) { s = s * 1664525u + 1013904223u; u += ((s >> 8) & 0xffff) / 65536.0f - 0.5f; } return u; };
  const float sc = 1.0f / sqrtf((float)dim / 3.0f);
  for (auto& x : hq) x = (_Float16)(rnd() * sc);
  _Float16 *slab, *q; float* ps; int* pr; unsigned long long* st;
  const int kp = 2 * crs::scan_wide_slots(k);
  hipMalloc(&slab, (size_t)rows * dim * 2); hipMalloc(&q, hq.size() * 2);
  hipMalloc(&ps, (size_t)nwg * nq * kp * 4); hipMalloc(&pr, (size_t)nwg * nq * kp * 4);
  const size_t nst = (size_t)nwg * nqb * nw * 12;
  hipMalloc(&st, nst * 8);
  const size_t n8 = (size_t)rows * dim / 8;   // dim is a multiple of 128
  fill_rows<<<dim3((unsigned)((n8 + 255) / 256)), dim3(256)>>>(slab, n8, sc);
  hipMemcpy(q, hq.data(), hq.size() * 2, hipMemcpyHostToDevice);
  crs::ScanArgs a{};
  a.q = q; a.slab = slab; a.part_scores = ps; a.part_rows = pr; a.stamps = st;
  a.n_rows = rows; a.n_tiles = n_tiles; a.nq = nq; a.k = k; a.kp = kp; a.nwg = nwg; a.nqb = nqb; a.sched = 2;
  a.t_dyn = n_tiles;
  unsigned* ticket = nullptr;
  const int slots = crs::scan_wide_slots(k);
  const int mfma = !crs::wide_has_16(dim, nw, slots) ? 32 : kn.wide_mfma ? kn.wide_mfma : crs::wide_default_mfma(dim, slots);
  a.no_stagger = kn.wide_stagger ? 0 : 1;
  a.no_defer = kn.wide_defer ? 0 : 1;
  const bool ring = kn.wide_ring && crs::wide_ring_form(dim, nw, slots, mfma);
  if (crs::scan_wide_streamed(k)) {   // the plan fields of plan.cpp's finish_plan
    a.nt = ((size_t)rows * dim * 2 >= ((size_t)1 << 30) && nqb == 1) ? 1 : 0;
    const int rounds = n_tiles / nwg;
    if (kn.wide_dyn && nqb == 1 && rounds >= 96) {
      int stat = (int)((long long)rounds * 15 / 100);
      if (stat < (ring ? 3 : 2)) stat = ring ? 3 : 2;
      hipMalloc(&ticket, 256);
      a.t_dyn = stat * nwg; a.ticket = ticket; a.dyn_mask = 7;
    }
  }
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  float ms = 0;
  for (int rep = 0; rep < 4; ++rep) {
    hipMemset(st, 0, nst * 8);
    if (ticket) hipMemset(ticket, 0, 4);
    hipEventRecord(e0, 0);
    int e = ring ? crs::scan_launch_wide_ring(a, dim, nw, mfma, 0) : crs::scan_launch_wide(a, dim, nw, mfma, 0);
    hipEventRecord(e1, 0);
    hipDeviceSynchronize();
    if (e) { printf("launch error %d\n", e); return 1; }
    hipEventElapsedTime(&ms, e0, e1);
  }
  std::vector<unsigned long long> hs(nst);
  hipMemcpy(hs.data(), st, nst * 8, hipMemcpyDeviceToHost);
  printf("rows %d dim %d nq %d k %d | waves/wg %d nqb %d streams %d tiles/stream %.1f nt %d tickets %s stagger-knob %s defer-knob %s mfma %d ring %d | kernel %.1f us (with stamps)\n", rows, dim, nq,
         k, nw, nqb, nwg, (double)n_tiles / nwg, a.nt, ticket ? "on" : "off", kn.wide_stagger ? "default" : "0", kn.wide_defer ? "default" : "0", mfma, (int)ring, ms * 1e3);
  // slots 2 / 4: the selection of waves 4..7 (deferred one tile) / of waves 0..3; 5: a count, not a lap; 8, 9: unused since the tile-best rewrite
  const char* names[12] = {"prologue", "tile-load issue", "selection (waves 4-7, deferred)", "MFMA sweep", "selection (waves 0-3)", "chain runs (a count)",
                           "wait next tile + LDS store", "barrier", "(unused)", "(unused)", "final flush", "TOTAL"};
  const size_t nwaves = nst / 12;
  // cycles per wave over the launch, and per tile of the wave's stream (mean); waves 0..3 and 4..7 of a workgroup apart
  const double tps = (double)n_tiles / nwg;
  for (int i = 0; i < 12; ++i) {
    std::vector<double> v; double half[2] = {0, 0}; size_t nh[2] = {0, 0};
    for (size_t w = 0; w < nwaves; ++w) {
      v.push_back((double)hs[w * 12 + i]);
      const int g = (nw == 8 && (w % nw) >= 4) ? 1 : 0;
      half[g] += (double)hs[w * 12 + i]; ++nh[g];
    }
    std::sort(v.begin(), v.end());
    double sum = 0; for (double x : v) sum += x;
    printf(i == 5 ? "  %-31s mean %9.0f  median %9.0f  max %9.0f | per tile: waves 0-3 %7.3f  waves 4-7 %7.3f\n"
                  : "  %-31s mean %9.0f  median %9.0f  max %9.0f | per tile: waves 0-3 %7.0f  waves 4-7 %7.0f\n",
           names[i], sum / nwaves, v[nwaves / 2], v.back(), half[0] / (nh[0] ? nh[0] : 1) / tps, half[1] / (nh[1] ? nh[1] : 1) / tps);
    if (i == 11) printf("  in-kernel clock (median TOTAL cycles / kernel time): %.3f GHz\n", v[nwaves / 2] / (ms * 1e6));
  }
  return 0;
}
