// Pillow's bicubic coefficient tables of one axis, built in double precision: what lib.clip_preprocess_tables hands the entries of
// csrc/clip_preprocess.hip and csrc/resize_u8.hip, restated for the stand-alone host checks of this directory.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

static double bicubic(double t) {
  const double a = -0.5;
  t = std::fabs(t);
  if (t < 1.0) return ((a + 2.0) * t - (a + 3.0)) * t * t + 1;
  if (t < 2.0) return (((t - 5) * t + 8) * t - 4) * a;
  return 0.0;
}

struct Axis {
  std::vector<int32_t> coef, bounds;
  int ksize;
};

static Axis make_axis(int I, int O) {
  Axis ax;
  if (I == O) {
    ax.ksize = 1;
    for (int x = 0; x < O; ++x) ax.coef.push_back(1 << 22), ax.bounds.push_back(x), ax.bounds.push_back(1);
    return ax;
  }
  const double scale = (double)I / O, fs = scale > 1.0 ? scale : 1.0, support = 2.0 * fs, ss = 1.0 / fs;
  ax.ksize = (int)std::ceil(support) * 2 + 1;
  ax.coef.assign((size_t)O * ax.ksize, 0);
  for (int xx = 0; xx < O; ++xx) {
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5), xmax = (int)(center + support + 0.5);
    if (xmin < 0) xmin = 0;
    if (xmax > I) xmax = I;
    xmax -= xmin;
    std::vector<double> w(xmax);
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += (w[x] = bicubic((x + xmin - center + 0.5) * ss));
    for (int x = 0; x < xmax; ++x) {
      const double k = ww != 0.0 ? w[x] / ww : w[x];
      ax.coef[(size_t)xx * ax.ksize + x] = k < 0 ? (int)(-0.5 + k * (1 << 22)) : (int)(0.5 + k * (1 << 22));
    }
    ax.bounds.push_back(xmin), ax.bounds.push_back(xmax);
  }
  return ax;
}
