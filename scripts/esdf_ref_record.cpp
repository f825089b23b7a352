// Records what the reference's own MapUtil<3>::updateESDF3d (src/path_searching/include/jps_collision/map_util.h:149-245) computes on two small maps, as raw
// data for tests/golden/refpin_esdf_*.npz (tests/test_esdf_cpu.py pins frx_map_esdf to them).  Run by hand where the reference tree is present; never by a test, by
// build() or on a GPU machine.  This file holds no text of the reference: it includes the header where it lies and calls it.
//
//   REF=<reference tree>/src/path_searching
//   g++ -O2 -march=x86-64-v3 -ffp-contract=off -std=c++14 -w -include cstdio -Ioracle/eigen_shim -Ioracle/boost_shim -Ioracle/ros_shim -I$REF/include -I$REF \
//       -o /tmp/esdf_ref_record scripts/esdf_ref_record.cpp && /tmp/esdf_ref_record /tmp/esdf_ref
//   python - <<'EOF'
//   import numpy as np
//   for k in (0, 1):
//       raw = open(f"/tmp/esdf_ref_{k}.bin", "rb").read()
//       dim = np.frombuffer(raw, np.int32, 3); res = np.frombuffer(raw, np.float64, 1, 16)[0]; n = int(dim.prod())
//       cells = np.frombuffer(raw, np.int8, n, 24); f = np.frombuffer(raw, np.float64, 3 * n, 24 + (n + 7) // 8 * 8).reshape(3, n)
//       np.savez_compressed(f"tests/golden/refpin_esdf_{k}.npz", dim=dim, res=res, cells=cells, pos=f[0], neg=f[1], all=f[2])
//   EOF
//
// File layout: int32 dim[3], 4 bytes of padding, float64 res, int8 cells[n] padded to a multiple of 8, float64 pos[n], neg[n], all[n].
#include <limits>   // (the header uses std::numeric_limits without including it)

#include <jps_collision/map_util.h>

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

static unsigned long long state = 0x9E3779B97F4A7C15ull;
static unsigned next_u32() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(state >> 33); }

static int record(const std::string &path, int nx, int ny, int nz, double res, int occupied_per_mille, int unknown_per_mille) {
    const size_t n = (size_t)nx * ny * nz;
    JPS::Tmap cells(n);
    for (size_t c = 0; c < n; c++) {
        const int r = (int)(next_u32() % 1000);
        cells[c] = r < occupied_per_mille ? 100 : r < occupied_per_mille + unknown_per_mille ? -1 : 0;
    }
    cells[0] = 100; cells[n - 1] = 0;                                    // both kinds of site, whatever the draw
    JPS::VoxelMapUtil map;
    map.setMap(Vec3f(0.0, 0.0, 0.0), Vec3i(nx, ny, nz), cells, res);
    map.distance_buffer_.assign(n, 10000.0); map.distance_buffer_neg_.assign(n, 10000.0); map.distance_buffer_all_.assign(n, 10000.0);
    map.tmp_buffer1_.assign(n, 0.0); map.tmp_buffer2_.assign(n, 0.0);
    map.updateESDF3d();
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) return 1;
    const int32_t head[4] = {nx, ny, nz, 0};
    std::fwrite(head, sizeof head, 1, f);
    std::fwrite(&res, sizeof res, 1, f);
    std::vector<signed char> padded((n + 7) / 8 * 8, 0);
    for (size_t c = 0; c < n; c++) padded[c] = cells[c];
    std::fwrite(padded.data(), 1, padded.size(), f);
    std::fwrite(map.distance_buffer_.data(), sizeof(double), n, f);
    std::fwrite(map.distance_buffer_neg_.data(), sizeof(double), n, f);
    std::fwrite(map.distance_buffer_all_.data(), sizeof(double), n, f);
    std::fclose(f);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: esdf_ref_record <output prefix>\n"); return 2; }
    const std::string prefix = argv[1];
    if (record(prefix + "_0.bin", 11, 7, 5, 0.1, 60, 150)) return 1;       // sparse obstacles, some unknown cells
    if (record(prefix + "_1.bin", 9, 13, 6, 0.3, 450, 250)) return 1;      // dense: thick obstacles, so neg reaches well past res
    return 0;
}
