// tests/clip_twin_main.cpp -- kvq_clip_host as a program of its own, for a run under AddressSanitizer and UBSan
// (tests/test_clip_host.py builds it with -fsanitize=address,undefined and runs it; nothing of it is loaded into python).
//   clip_twin_main TEXT OUT PROBE [PROBE ...]
// The text is read into a heap block of exactly its size -- a byte read or written behind the text's last byte, or in front of its
// first, is the sanitizer's to report --, masked twice as one chunk (the second time must change nothing), and written to OUT
// with the eight words of the first run behind it.
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
    if (argc < 4 || argc > 3 + KVQ_ADAPT_MAX_PROBES) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    fseek(f, 0, SEEK_END); const long n = ftell(f); fseek(f, 0, SEEK_SET);
    uint8_t *text = (uint8_t *)malloc((size_t)n);
    if (!text || fread(text, 1, (size_t)n, f) != (size_t)n) return 3;
    fclose(f);
    const uint8_t *probes[KVQ_ADAPT_MAX_PROBES]; int32_t lens[KVQ_ADAPT_MAX_PROBES];
    const int32_t np = argc - 3;
    for (int32_t k = 0; k < np; k++) { probes[k] = (const uint8_t *)argv[3 + k]; lens[k] = (int32_t)strlen(argv[3 + k]); }
    const int64_t co[2] = { 0, n };
    int64_t words[KVQ_CLIP_WORDS] = { 0 }, again[KVQ_CLIP_WORDS] = { 0 };
    if (kvq_clip_host(text, n, co, 1, probes, lens, np, words)) return 4;
    uint8_t *once = (uint8_t *)malloc((size_t)n);
    memcpy(once, text, (size_t)n);
    if (kvq_clip_host(text, n, co, 1, probes, lens, np, again)) return 4;
    if (memcmp(once, text, (size_t)n) || memcmp(words, again, sizeof(words))) return 5;      // idempotent, bytes and words
    FILE *o = fopen(argv[2], "wb");
    if (!o || fwrite(text, 1, (size_t)n, o) != (size_t)n || fwrite(words, 8, KVQ_CLIP_WORDS, o) != KVQ_CLIP_WORDS) return 6;
    fclose(o);
    free(once); free(text);
    return 0;
}
