// tests/deflate_twin_main.cpp -- kvq_deflate_bgzf_host as a program of its own, for a run under AddressSanitizer and UBSan
// (tests/test_deflate_host.py builds it with -fsanitize=address,undefined and runs it; nothing of it is loaded into python).
//   deflate_twin_main TEXT OUT
// The text is read into a heap block of exactly its size, so that its input ends with the text's last byte, and deflated into a heap
// block of exactly kvq_deflate_bound bytes -- a byte read behind the text or in front of it, or written outside the output, is the
// sanitizer's to report.  OUT gets BGZF(text) with the eight words behind it.
#include "../kvarq_amd/csrc/kvq_twins.cpp"
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

void kvq_set_error(int code, const char *fmt, ...)
{
    va_list ap; va_start(ap, fmt);
    fprintf(stderr, "error %d: ", code); vfprintf(stderr, fmt, ap); fputc('\n', stderr);
    va_end(ap);
}
void kvq_clear_error() {}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    fseek(f, 0, SEEK_END); const long n = ftell(f); fseek(f, 0, SEEK_SET);
    uint8_t *text = (uint8_t *)malloc((size_t)n ? (size_t)n : 1);
    if (!text || fread(text, 1, (size_t)n, f) != (size_t)n) return 3;
    fclose(f);
    const int64_t cap = kvq_deflate_bound(n);
    uint8_t *out = (uint8_t *)malloc((size_t)cap ? (size_t)cap : 1);
    if (!out) return 3;
    int64_t words[KVQ_DEFLATE_WORDS];
    const int64_t got = kvq_deflate_bgzf_host(text, n, out, cap, words);
    if (got < 0 || got != words[KVQ_DEFLATE_BYTES_OUT] || n != words[KVQ_DEFLATE_BYTES_IN]) return 4;
    // a buffer one byte short of what the text takes is refused, and nothing is written behind it
    if (got > 0) {
        uint8_t *tight = (uint8_t *)malloc((size_t)got - 1 ? (size_t)got - 1 : 1);
        int64_t w2[KVQ_DEFLATE_WORDS];
        if (kvq_deflate_bgzf_host(text, n, tight, got - 1, w2) != -1) return 5;
        free(tight);
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o || fwrite(out, 1, (size_t)got, o) != (size_t)got || fwrite(words, 8, KVQ_DEFLATE_WORDS, o) != KVQ_DEFLATE_WORDS) return 6;
    fclose(o);
    free(out); free(text);
    return 0;
}
