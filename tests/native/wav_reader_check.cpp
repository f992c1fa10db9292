// Stand-alone driver of the native WAV reader (pfann_amd/csrc/wavio.hip, host code only), meant to be built with
// -fsanitize=address,undefined together with that file (tests/test_pcm_host.py does so):
//   wav_reader_check FILE...
// probes the files on two threads, reads them on two threads into a heap buffer of EXACTLY the probed size, so that a
// single sample written past a file's share is a heap-buffer-overflow, and prints "<path> <samples read, -1 if refused>
// <status>" per file.  Exit status 0 unless the reader misbehaves (the sanitizers end the process on their own findings).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "pfann_amd.h"

int main(int argc, char **argv) {
    const int n = argc - 1;
    if (n < 1) { fprintf(stderr, "usage: %s FILE...\n", argv[0]); return 2; }
    const char *const *paths = argv + 1;
    std::vector<pfann_wav_info> info(n);
    if (pfann_wav_probe(paths, n, 2, info.data()) != 0) { fprintf(stderr, "probe failed\n"); return 1; }
    std::vector<int64_t> off(n);
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        off[i] = total;
        if (info[i].status == 0) {
            if (info[i].n_frames < 0 || info[i].n_ch < 1 || info[i].data_pos < 12) { fprintf(stderr, "%s: bad probe\n", paths[i]); return 1; }
            total += info[i].n_frames * info[i].n_ch;
        }
    }
    // a capacity one sample short is refused before anything is written
    std::vector<pfann_wav_info> again(info);
    int16_t *dst = new int16_t[total > 0 ? total : 1];
    if (total > 0 && pfann_wav_read(paths, n, 2, again.data(), off.data(), dst, total - 1) != -2) { fprintf(stderr, "a slab one sample short was accepted\n"); return 1; }
    if (pfann_wav_read(paths, n, 2, info.data(), off.data(), dst, total) != 0) { fprintf(stderr, "read failed\n"); return 1; }
    int64_t sum = 0;
    for (int64_t i = 0; i < total; ++i) sum += dst[i];              // every sample was written (MemorySanitizer's job, kept cheap)
    for (int i = 0; i < n; ++i)
        printf("%s %lld %d\n", paths[i], info[i].status == 0 ? (long long)(info[i].n_frames * info[i].n_ch) : -1LL, (int)info[i].status);
    printf("total %lld checksum %lld\n", (long long)total, (long long)sum);
    delete[] dst;
    // no files at all, and refused arguments
    if (pfann_wav_probe(paths, 0, 2, nullptr) != 0 || pfann_wav_probe(nullptr, 1, 1, info.data()) != -1) { fprintf(stderr, "argument checks\n"); return 1; }
    return 0;
}
