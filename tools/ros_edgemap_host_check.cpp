// Stand-alone run of the host packer rebvo::pack_ros_edgemap (rebvo_amd/host/src/ros_edgemap.cpp), for a sanitizer build on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Irebvo_amd/host/include -Iinclude \
//       tools/ros_edgemap_host_check.cpp rebvo_amd/host/src/ros_edgemap.cpp -o ros_edgemap_host_check
// stdin : int32 kn; double K, zfm; kn x 168-byte KeyLines      stdout: kn x 12-byte points; kn x 52-byte records
// The buffers are heap arrays of exactly kn entries, so a write past either end is a sanitizer report.
#include <cstdio>
#include <cstdint>
#include <memory>

#include "rebvo/ros_edgemap.h"

int main() {
    int32_t kn;
    double K, zfm;
    if (fread(&kn, 4, 1, stdin) != 1 || fread(&K, 8, 1, stdin) != 1 || fread(&zfm, 8, 1, stdin) != 1 || kn < 0) return 2;
    std::unique_ptr<rebvo::KeyLine[]> kl(new rebvo::KeyLine[kn]);
    std::unique_ptr<rebvo::ros_point[]> p(new rebvo::ros_point[kn]);
    std::unique_ptr<rebvo::ros_keyline[]> k(new rebvo::ros_keyline[kn]);
    if (kn > 0 && fread(kl.get(), sizeof(rebvo::KeyLine), kn, stdin) != (size_t)kn) return 3;
    rebvo::pack_ros_edgemap(kl.get(), kn, K, zfm, p.get(), k.get());
    rebvo::pack_ros_edgemap(kl.get(), kn, K, zfm, nullptr, k.get());
    rebvo::pack_ros_edgemap(kl.get(), kn, K, zfm, p.get(), nullptr);
    fwrite(p.get(), sizeof(rebvo::ros_point), kn, stdout);
    fwrite(k.get(), sizeof(rebvo::ros_keyline), kn, stdout);
    return 0;
}
