"""Generates tests/golden/golden_deploy.npz: what the reference's OWN ncnn sample class returns for chosen export maps.

Runs only where the reference tree is present.  Nothing of the sample is copied: the generator writes two stub headers of its own
into a temporary directory (net.h: an ncnn::Mat that is {w, h, c, data, channel()} with Net / Extractor no-ops; opencv2/opencv.hpp:
a cv::Mat that holds cols, rows, data), compiles sample/ncnn/src/yolo-fastestv2.cpp IN PLACE with g++ -O0 next to a small driver
that reaches the class's private predHandle / nmsHandle through `#define private public`, feeds it the maps of every case and
records the boxes it returns.  The binary lives and dies in the temporary directory.

    python tests/golden/make_golden_deploy.py [--reference /root/reference] [--seed 7]

Every case is checked to be free of score ties among its candidates (a tie makes the sample's own output depend on std::sort's
whim): regenerate with another seed if the assertion fires.
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import deploy_model  # noqa: E402  (only its candidate stage, for the tie check)

NET_H = r"""
#pragma once
#include <cassert>
#include <cstdio>
#include <cstring>
namespace ncnn {
struct Mat {
  int w = 0, h = 0, c = 0; const float* data = nullptr;
  enum { PIXEL_BGR = 2 };
  const float* channel(int q) const { return data + (size_t)q * h * w; }
  static Mat from_pixels_resize(const unsigned char*, int, int, int, int, int) { return Mat(); }
  void substract_mean_normalize(const float*, const float*) {}
};
struct Extractor { void set_num_threads(int) {} int input(const char*, const Mat&) { return 0; } int extract(const char*, Mat&) { return 0; } };
struct Net { int load_param(const char*) { return 0; } int load_model(const char*) { return 0; } Extractor create_extractor() { return Extractor(); } };
}
"""
OPENCV_H = r"""
#pragma once
namespace cv { struct Mat { int cols = 0, rows = 0; unsigned char* data = nullptr; }; }
"""
DRIVER = r"""
#define private public
#include "yolo-fastestv2.h"
#undef private
#include <cstdlib>
// in:  int32 in_h, in_w, classes, fh0, fw0, fh1, fw1 | float anchors[12], thresh, nms, scaleW, scaleH | map0 | map1
// out: int32 n | n x {int32 x1, y1, x2, y2, cate; float score}
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb");
  int hd[7]; float fl[16];
  if (!f || fread(hd, 4, 7, f) != 7 || fread(fl, 4, 16, f) != 16) return 2;
  const int C = 15 + hd[2];
  std::vector<float> m0((size_t)hd[3] * hd[4] * C), m1((size_t)hd[5] * hd[6] * C);
  if (fread(m0.data(), 4, m0.size(), f) != m0.size() || fread(m1.data(), 4, m1.size(), f) != m1.size()) return 3;
  fclose(f);
  yoloFastestv2 api;
  api.inputHeight = hd[0]; api.inputWidth = hd[1]; api.numCategory = hd[2]; api.nmsThresh = fl[13];
  api.anchor.assign(fl, fl + 12);
  ncnn::Mat out[2];
  out[0].c = hd[3]; out[0].h = hd[4]; out[0].w = C; out[0].data = m0.data();
  out[1].c = hd[5]; out[1].h = hd[6]; out[1].w = C; out[1].data = m1.data();
  std::vector<TargetBox> tmp, dst;
  api.predHandle(out, tmp, fl[14], fl[15], fl[12]);
  api.nmsHandle(tmp, dst);
  FILE* g = fopen(argv[2], "wb");
  int n = (int)dst.size();
  fwrite(&n, 4, 1, g);
  for (auto& b : dst) { int v[5] = {b.x1, b.y1, b.x2, b.y2, b.cate}; fwrite(v, 4, 5, g); fwrite(&b.score, 4, 1, g); }
  fclose(g);
  return 0;
}
"""

COCO_ANCHORS = [12.64, 19.39, 37.88, 51.48, 55.71, 138.31, 126.91, 78.23, 131.57, 214.55, 279.92, 258.87]


def softmax32(x, axis):
    e = np.exp((x - x.max(axis, keepdims=True)).astype(np.float32)).astype(np.float32)
    return (e / e.sum(axis, keepdims=True, dtype=np.float32)).astype(np.float32)


def sigmoid32(x):
    return (np.float32(1) / (np.float32(1) + np.exp(-x.astype(np.float32)))).astype(np.float32)


def random_maps(rng, in_h, in_w, classes, obj_lo=0.0, spread=1.0):
    maps = []
    for d in (16, 32):
        fh, fw = in_h // d, in_w // d
        reg = (0.5 + spread * (rng.random((fh, fw, 12)) - 0.5)).astype(np.float32)
        obj = (obj_lo + (1 - obj_lo) * rng.random((fh, fw, 3))).astype(np.float32)
        cls = softmax32((3 * rng.standard_normal((fh, fw, classes))).astype(np.float32), -1)
        maps.append(np.concatenate([reg, obj, cls], -1))
    return maps


def hand_maps():
    """32x32, 3 classes, anchors all (16, 16): 2x2 cells at stride 16 and one at stride 32, every row made by hand"""
    m0 = np.zeros((2, 2, 18), np.float32)
    m1 = np.zeros((1, 1, 18), np.float32)

    def row(m, y, x, b, reg, obj, cls=None):
        m[y, x, 4 * b:4 * b + 4] = reg
        m[y, x, 12 + b] = obj
        if cls is not None:
            m[y, x, 15:] = cls
    # cell (0,0) and (0,1), class 0: anchor 0 boxes [0,16] and [16,32] touch along x = 16 (inter width 0: kept);
    # anchor 1: two zero-area boxes at the same point (0 / 0: kept); anchor 2 of (0,0): centre at -8, x1 = -13.12 -> -13 (toward zero)
    row(m0, 0, 0, 0, [0.5, 0.5, 0.5, 0.5], 0.90, [0.8, 0.15, 0.05])
    row(m0, 0, 1, 0, [0.5, 0.5, 0.5, 0.5], 0.85, [0.7, 0.2, 0.1])
    row(m0, 0, 0, 1, [0.75, 0.75, 0.0, 0.0], 0.80)
    row(m0, 0, 1, 1, [0.25, 0.75, 0.0, 0.0], 0.75)
    row(m0, 0, 0, 2, [0.0, 0.0, 0.4, 0.4], 0.70)
    row(m0, 0, 1, 2, [0.5, 0.5, 0.45, 0.55], 0.65)        # overlaps anchor 0 of its cell heavily, same class: suppressed
    # cell (1,0): obj 0 on anchor 0 -> cls * obj == 0, never a candidate; anchors 1, 2 of another class overlap the rows above freely
    row(m0, 1, 0, 0, [0.5, 0.5, 0.5, 0.5], 0.0, [0.1, 0.6, 0.3])
    row(m0, 1, 0, 1, [0.5, 0.1, 0.6, 0.6], 0.95)
    row(m0, 1, 0, 2, [0.5, 0.12, 0.62, 0.58], 0.60)
    # cell (1,1): all-zero class vector -> nothing above 0 for any anchor
    row(m0, 1, 1, 0, [0.5, 0.5, 0.5, 0.5], 0.99, [0.0, 0.0, 0.0])
    row(m0, 1, 1, 1, [0.5, 0.5, 0.5, 0.5], 0.98)
    row(m0, 1, 1, 2, [0.5, 0.5, 0.5, 0.5], 0.97)
    # scale 1: a big box over everything (class 2), one that leaves the frame on the negative side, one below the threshold
    row(m1, 0, 0, 0, [0.5, 0.5, 0.7, 0.7], 0.55, [0.05, 0.05, 0.9])
    row(m1, 0, 0, 1, [0.1, 0.1, 0.9, 0.9], 0.50)
    row(m1, 0, 0, 2, [0.5, 0.5, 0.5, 0.5], 0.05)
    return m0, m1


def build_cases(seed, golden_real):
    rng = np.random.default_rng(seed)
    cases = {}

    def add(name, maps, in_h, in_w, classes, anchors, thresh, nms, sw=1.0, sh=1.0):
        cases[name] = dict(map0=maps[0], map1=maps[1], hw=np.array([in_h, in_w, classes], np.int32), anchors=np.array(anchors, np.float64),
                           par=np.array([thresh, nms, sw, sh], np.float32))
    for nc in (1, 4, 80):
        add("s32_c%d" % nc, random_maps(rng, 32, 32, nc), 32, 32, nc, COCO_ANCHORS, 0.05, 0.25)
    add("s64x96_c5", random_maps(rng, 64, 96, 5), 64, 96, 5, COCO_ANCHORS, 0.1, 0.25, 1.5, 0.75)
    z = np.load(golden_real)
    real = []
    for s in ("2", "3"):   # the export layout of image 0's logits (model/detector.py:33-44), computed here in numpy: input DATA for the sample
        reg, obj, cls = z["logit_reg" + s][0], z["logit_obj" + s][0], z["logit_cls" + s][0]
        real.append(np.ascontiguousarray(np.concatenate([sigmoid32(reg), sigmoid32(obj), softmax32(cls, 0)], 0).transpose(1, 2, 0)))
    add("real352_c80", real, 352, 352, 80, COCO_ANCHORS, 0.01, 0.25, 640 / 352, 480 / 352)
    add("dense128_c2", random_maps(rng, 128, 128, 2, obj_lo=0.3, spread=0.3), 128, 128, 2, COCO_ANCHORS, 0.0, 0.25)
    add("hand32_c3", hand_maps(), 32, 32, 3, [16.0] * 12, 0.3, 0.25, 1.5, 0.75)
    add("hand32_c3_unit", hand_maps(), 32, 32, 3, [16.0] * 12, 0.3, 0.25)
    return cases


def run_sample(exe, tmp, c):
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    in_h, in_w, nc = (int(v) for v in c["hw"])
    with open(fin, "wb") as f:
        np.array([in_h, in_w, nc, c["map0"].shape[0], c["map0"].shape[1], c["map1"].shape[0], c["map1"].shape[1]], np.int32).tofile(f)
        np.concatenate([c["anchors"].astype(np.float32), c["par"]]).astype(np.float32).tofile(f)
        np.ascontiguousarray(c["map0"], np.float32).tofile(f)
        np.ascontiguousarray(c["map1"], np.float32).tofile(f)
    subprocess.run([exe, fin, fout], check=True, stdout=subprocess.DEVNULL)
    raw = np.fromfile(fout, np.int32)
    return raw[1:].reshape(int(raw[0]), 6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    src = os.path.join(args.reference, "sample", "ncnn", "src")
    cases = build_cases(args.seed, os.path.join(HERE, "golden_real.npz"))
    out = {"cases": np.array(sorted(cases))}
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "opencv2"))
        for name, text in (("net.h", NET_H), (os.path.join("opencv2", "opencv.hpp"), OPENCV_H), ("driver.cpp", DRIVER)):
            with open(os.path.join(tmp, name), "w") as f:
                f.write(text)
        exe = os.path.join(tmp, "sample_driver")
        subprocess.run(["g++", "-O0", "-w", "-I", tmp, "-I", os.path.join(src, "include"), os.path.join(tmp, "driver.cpp"),
                        os.path.join(src, "yolo-fastestv2.cpp"), "-o", exe], check=True)
        for name, c in sorted(cases.items()):
            in_h = int(c["hw"][0])
            thresh, nms, sw, sh = (float(v) for v in c["par"])
            scores = np.concatenate([deploy_model.candidates(m, s, c["anchors"], in_h, thresh, sw, sh)[2] for s, m in enumerate((c["map0"], c["map1"]))])
            assert len(np.unique(scores)) == len(scores), "%s: two candidates share a score - use another --seed" % name
            rec = run_sample(exe, tmp, c)
            print("%-16s %4d candidates -> %4d boxes" % (name, len(scores), len(rec)))
            for k, v in c.items():
                out["%s_%s" % (name, k)] = v
            out["%s_rec" % name] = rec
    path = os.path.join(HERE, "golden_deploy.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
