// Stand-alone run of the mirror library's key-frame file code (rebvo_amd/host/include/rebvo/keyframe.h: header only, no device), for
// tests/test_keyframe_file_cpu.py and for a sanitizer build on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Irebvo_amd/host/include -Iinclude \
//       tools/keyframe_file_host_check.cpp -o keyframe_file_host_check
//   keyframe_file_host_check IN OUT   loadKeyframesFromFile(IN) -> saveKeyframes2File(OUT); prints "<kfnum> <kn> <kn> ..."
// Exit status 0, 3 when IN does not load (a truncated file), 4 when OUT cannot be written.
#include <cstdio>
#include <vector>

#include "rebvo/keyframe.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    std::vector<rebvo::keyframe> list;
    if (!rebvo::keyframe::loadKeyframesFromFile(argv[1], list)) {
        printf("load failed after %zu key frames\n", list.size());
        return 3;
    }
    printf("%zu", list.size());
    for (const rebvo::keyframe &kf : list) printf(" %d", kf.KNum());
    printf("\n");
    return rebvo::keyframe::saveKeyframes2File(argv[2], list) ? 0 : 4;
}
