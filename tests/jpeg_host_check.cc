// Stand-alone robustness run of the JPEG host stage (grit_amd/csrc/jpeg_host.h), built by tests/test_jpeg_cpu.py with
// -fsanitize=address,undefined.  Input: a container  u32 n, then per file  u32 flags (1: expected to decode, 2: mutate),
// u32 length, bytes.  Every file runs once; a file marked 2 also runs as every truncation prefix and with every byte
// replaced in turn by 0x00, 0xFF and byte ^ 0x55.  Inputs and outputs live in heap blocks of their exact size, so a read
// or write past either is a sanitizer report.  Exit 0: every call returned a status, and the status of each whole file
// is the expected one.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../grit_amd/csrc/jpeg_host.h"

static long calls = 0, decoded = 0;

static int run(const uint8_t* bytes, long n) {  // GRIT_OK only when both stages accept
    uint8_t* data = (uint8_t*)malloc(n ? n : 1);
    memcpy(data, bytes, n);
    grit_jpeg::Header h;
    int st = grit_jpeg::parse_header(data, n, &h);
    if (st == GRIT_OK) {
        int16_t* coef = (int16_t*)malloc(h.info.coef_bytes);  // a mutated size field may ask for much; only decoded blocks are touched
        st = coef ? grit_jpeg::entropy(data, n, &h.info, coef, h.info.coef_bytes) : GRIT_ERR_UNSUPPORTED;
        free(coef);
    }
    free(data);
    ++calls;
    if (st != GRIT_OK && st != GRIT_ERR_UNSUPPORTED) {
        fprintf(stderr, "unexpected status %d\n", st);
        exit(2);
    }
    decoded += st == GRIT_OK;
    return st;
}

int main(int argc, char** argv) {
    if (argc != 2) return 3;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    uint32_t n = 0;
    if (fread(&n, 4, 1, f) != 1) return 3;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t head[2];
        if (fread(head, 4, 2, f) != 2) return 3;
        const long len = head[1];
        uint8_t* bytes = (uint8_t*)malloc(len ? len : 1);
        if (fread(bytes, 1, len, f) != (size_t)len) return 3;
        const int st = run(bytes, len);
        if ((st == GRIT_OK) != ((head[0] & 1) != 0)) {
            fprintf(stderr, "file %u: status %d, expected %s\n", i, st, (head[0] & 1) ? "ok" : "unsupported");
            return 4;
        }
        if (head[0] & 2) {
            for (long cut = 0; cut < len; ++cut) run(bytes, cut);
            for (long at = 0; at < len; ++at) {
                const uint8_t keep = bytes[at];
                const uint8_t with[3] = {0x00, 0xFF, (uint8_t)(keep ^ 0x55)};
                for (int k = 0; k < 3; ++k) {
                    bytes[at] = with[k];
                    run(bytes, len);
                }
                bytes[at] = keep;
            }
        }
        free(bytes);
    }
    fclose(f);
    printf("calls %ld decoded %ld\n", calls, decoded);
    return 0;
}
