// sift_batch_plan_asan_main.cpp — sift_batch_plan.h (the plan of cvDetectFeaturesBatch) as a stand-alone
// program for AddressSanitizer + UBSan (tests/test_sift_batch.py builds and runs it; nothing is loaded
// into Python). Input: one line per batch, "mode nImages", the six SiftConfig fields in their order, the
// number of groups, then per group "count w h channels reserved" (count images of that shape in a row;
// nImages may differ from their sum only where the plan refuses nImages before it reads an image). No
// pixel is read by a plan: every image points at one byte. Output per batch: "ok" and the eight numbers
// of mcvTestSiftBatchPlan, or "refused: " and the message; then the size arithmetic's overflow refusals
// and a final "sift_batch_plan_asan ok" line.
#include "sift_batch_plan.h"

#include <fstream>
#include <iostream>
#include <sstream>

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string line;
    int batches = 0;
    const uint8_t pixel = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ls(line);
        int mode = 0, nImages = 0, groups = 0;
        mcv::SiftConfigIn cfg = {};
        ls >> mode >> nImages >> cfg.FeatureCount >> cfg.OctaveLayers >> cfg.ContrastThreshold >> cfg.EdgeThreshold >>
            cfg.Sigma >> cfg.DescriptorType >> groups;
        if (!ls || groups < 0) return 3;
        std::vector<mcv::SiftImageIn> images;
        for (int g = 0; g < groups; ++g) {
            int count = 0;
            mcv::SiftImageIn im = {&pixel, 0, 0, 0, 0};
            ls >> count >> im.width >> im.height >> im.channels >> im.reserved;
            if (!ls || count < 0) return 3;
            images.insert(images.end(), (size_t)count, im);
        }
        if (nImages >= 0 && nImages <= mcv::kSiftBatchMaxImages && (size_t)nImages != images.size()) return 3;
        mcv::SiftBatchPlan B;
        std::string err;
        if (mcv::sift_batch_plan("plan", images.empty() ? nullptr : images.data(), nImages, mode, &cfg, B, err)) {
            long long v[8];
            mcv::sift_batch_plan_out8(B, v);
            std::cout << "ok";
            for (long long x : v) std::cout << " " << x;
            std::cout << "\n";
            // the table is consistent with itself: buckets and offsets ascend, every octave inside the pyramid
            size_t bucket = 0;
            for (const mcv::SiftBatchImage& T : B.table) {
                if ((size_t)T.bucketBegin != bucket || T.bucketEnd < T.bucketBegin) return 5;
                bucket = (size_t)T.bucketEnd;
                for (int o = 0; o < T.nOctaves; ++o) {
                    const size_t end = T.obase[o] + (size_t)(B.cfg.P.nl + 3) * (size_t)T.ow[o] * (size_t)T.oh[o];
                    if (end > B.pyramidFloats || T.rowBase[o] < T.bucketBegin || T.rowBase[o] >= T.bucketEnd) return 5;
                }
                if (T.nOctaves > 0 && T.scratchOff + (size_t)T.ow[0] * (size_t)T.oh[0] > B.scratchFloats) return 5;
                if (T.imgOff + (size_t)T.w * (size_t)T.h * (size_t)T.ch > B.imgBytes) return 5;
            }
            if (bucket != (size_t)B.nBuckets) return 5;
        } else {
            std::cout << "refused: " << err << "\n";
        }
        ++batches;
    }
    size_t out = 0;
    const size_t big = ~(size_t)0;
    if (mcv::sift_size_add(big, 1, out) || mcv::sift_size_add(big - 3, 4, out) || mcv::sift_size_mul(big / 2 + 1, 2, out) ||
        mcv::sift_size_mul((size_t)1 << 33, (size_t)1 << 31, out))
        return 6;
    if (!mcv::sift_size_add(big - 3, 3, out) || out != big || !mcv::sift_size_mul((size_t)1 << 32, (size_t)1 << 31, out) ||
        out != (size_t)1 << 63)
        return 6;
    std::cout << "overflow refused: 4, kept: 2\n";
    std::cout << "sift_batch_plan_asan ok: " << batches << " batches\n";
    return 0;
}
