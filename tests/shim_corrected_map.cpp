// FastLioSamQn's corrected-map rebuild (fast_lio_sam_qn.cpp:302-316, 398-411, 435-448) written against qn_map::CorrectedMap:
// keyframes added one by one as PointXYZI clouds, then one build with the corrected poses.
// usage: shim_corrected_map keyframes.bin poses.bin leaf out.bin
//   keyframes.bin: per keyframe uint32 n, then n x (x, y, z, intensity) float32; poses.bin: one row-major 4x4 float64 per keyframe
//   out.bin: the map as n x (x, y, z, intensity) float32, read back from the PointXYZI records; prints the point count
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <qn_map/corrected_map.hpp>

using PointType = pcl::PointXYZI;

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  qn_map::CorrectedMap<PointType> map;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  uint32_t n = 0;
  while (std::fread(&n, 4, 1, f) == 1) {
    pcl::PointCloud<PointType> c;
    for (uint32_t i = 0; i < n; i++) {
      float v[4];
      if (std::fread(v, 4, 4, f) != 4) return 4;
      PointType p; p.x = v[0]; p.y = v[1]; p.z = v[2]; p.intensity = v[3]; c.push_back(p);
    }
    map.addKeyframe(c);
  }
  std::fclose(f);
  std::vector<Eigen::Matrix4d> poses;
  f = std::fopen(argv[2], "rb");
  if (!f) return 3;
  double T[16];
  while (std::fread(T, 8, 16, f) == 16) { Eigen::Matrix4d M; for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) M(r, c) = T[4 * r + c]; poses.push_back(M); }
  std::fclose(f);
  pcl::PointCloud<PointType> out;
  map.build(poses, (float)std::atof(argv[3]), out);
  f = std::fopen(argv[4], "wb");
  if (!f) return 3;
  for (size_t i = 0; i < out.size(); i++) { const float v[4] = {out[i].x, out[i].y, out[i].z, out[i].intensity}; std::fwrite(v, 4, 4, f); }
  std::fclose(f);
  std::printf("%zu\n", out.size());
  return 0;
}
