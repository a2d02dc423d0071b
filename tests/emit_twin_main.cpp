// tests/emit_twin_main.cpp -- kvq_emit_host as a program of its own, for a run under AddressSanitizer and UBSan
// (tests/test_emit_host.py builds it with -fsanitize=address,undefined and runs it; nothing of it is loaded into python).
//   emit_twin_main TEXT OUT AMIN MIN_LENGTH
// The text is read into a heap block of exactly its size, and emitted as one chunk into a heap block of exactly nbytes + nrec
// bytes -- a byte read behind the text's last byte or in front of its first, or written outside the output, is the sanitizer's
// to report.  OUT gets the emitted text with the eight words behind it.
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
    if (argc != 5) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    fseek(f, 0, SEEK_END); const long n = ftell(f); fseek(f, 0, SEEK_SET);
    uint8_t *text = (uint8_t *)malloc((size_t)n);
    if (!text || fread(text, 1, (size_t)n, f) != (size_t)n) return 3;
    fclose(f);
    int64_t newlines = 0;
    for (long i = 0; i < n; i++) newlines += text[i] == '\n';
    const int64_t cap = n + newlines / 4;
    uint8_t *out = (uint8_t *)malloc((size_t)cap);
    if (!out) return 3;
    const int64_t co[2] = { 0, n };
    int64_t words[KVQ_EMIT_WORDS] = { 0 };
    const int64_t got = kvq_emit_host(text, n, co, 1, atoi(argv[3]), atoi(argv[4]), out, cap, words);
    if (got < 0 || got != words[KVQ_EMIT_BYTES_OUT]) return 4;
    // a buffer one byte short of what the text emits is refused, and nothing is written behind it
    if (got > 0) {
        uint8_t *tight = (uint8_t *)malloc((size_t)got - 1);
        int64_t w2[KVQ_EMIT_WORDS] = { 0 };
        if (kvq_emit_host(text, n, co, 1, atoi(argv[3]), atoi(argv[4]), tight, got - 1, w2) != -1) return 5;
        free(tight);
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o || fwrite(out, 1, (size_t)got, o) != (size_t)got || fwrite(words, 8, KVQ_EMIT_WORDS, o) != KVQ_EMIT_WORDS) return 6;
    fclose(o);
    free(out); free(text);
    return 0;
}
