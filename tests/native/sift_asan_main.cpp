// sift_asan_main.cpp — sift_ref.h (the host twin of cvDetectFeatures) as a stand-alone program for
// AddressSanitizer + UBSan (tests/test_sift.py builds and runs it; nothing is loaded into Python).
// Input: one line per grey image, "w h", the six SiftConfig fields in their order (FeatureCount,
// OctaveLayers, ContrastThreshold, EdgeThreshold, Sigma, DescriptorType) and the w h bytes. Output per
// image: the keypoint count, then per keypoint the 7 KeyPoint2d words (as unsigned integers) and the
// 128 descriptor bytes; a final "sift_asan ok" line.
#include "sift_ref.h"

#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    int cases = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ls(line);
        int w = 0, h = 0;
        mcv::SiftConfigIn cfg = {};
        ls >> w >> h >> cfg.FeatureCount >> cfg.OctaveLayers >> cfg.ContrastThreshold >> cfg.EdgeThreshold >>
            cfg.Sigma >> cfg.DescriptorType;
        if (!ls || w <= 0 || h <= 0) return 3;
        std::vector<uint8_t> img((size_t)w * (size_t)h);
        for (auto& b : img) {
            int v = 0;
            ls >> v;
            b = (uint8_t)v;
        }
        if (!ls) return 3;
        mcv::SiftPlan S;
        std::string err;
        if (!mcv::sift_plan("sift_asan", img.data(), w, h, 1, 4, &cfg, S, err)) {
            std::cerr << err << "\n";
            return 4;
        }
        mcv::SiftHostResult R;
        mcv::sift_host_detect(img.data(), S, R);
        std::cout << R.recs.size() << "\n";
        for (size_t i = 0; i < R.recs.size(); ++i) {
            const mcv::SiftRec& q = R.recs[i];
            const float f[5] = {q.x, q.y, q.size, q.angle, q.response};
            for (float v : f) {
                uint32_t u;
                std::memcpy(&u, &v, 4);
                std::cout << u << " ";
            }
            std::cout << (uint32_t)q.octave << " " << 0xffffffffu;
            for (int k = 0; k < mcv::kSiftDescLen; ++k)
                std::cout << " " << (int)mcv::sift_desc_byte(R.desc[i * (size_t)mcv::kSiftDescLen + (size_t)k]);
            std::cout << "\n";
        }
        ++cases;
    }
    std::cout << "sift_asan ok: " << cases << " cases\n";
    return 0;
}
