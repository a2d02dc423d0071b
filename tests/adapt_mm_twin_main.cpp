// tests/adapt_mm_twin_main.cpp -- kvq_adapt_host_mm and kvq_clip_host_mm as a program of its own, for a run under AddressSanitizer
// and UBSan (tests/test_adapt_mm_host.py builds it with -fsanitize=address,undefined and runs it; nothing of it is loaded into
// python).
//   adapt_mm_twin_main TEXT OUT PER PROBE [PROBE ...]
// The text is read into a heap block of exactly its size -- a window that hangs over the last line's end, or a byte read behind
// the text's last byte or in front of its first, is the sanitizer's to report --, counted by kvq_adapt_host_mm, masked twice by
// kvq_clip_host_mm as one chunk (the second time must change nothing), and written to OUT with the adapters array and the eight
// words of the first mask behind it.
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
    if (argc < 5 || argc > 4 + KVQ_ADAPT_MAX_PROBES) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    fseek(f, 0, SEEK_END); const long n = ftell(f); fseek(f, 0, SEEK_SET);
    uint8_t *text = (uint8_t *)malloc((size_t)n);
    if (!text || fread(text, 1, (size_t)n, f) != (size_t)n) return 3;
    fclose(f);
    const int32_t per = (int32_t)atoi(argv[3]);
    const uint8_t *probes[KVQ_ADAPT_MAX_PROBES]; int32_t lens[KVQ_ADAPT_MAX_PROBES];
    const int32_t np = argc - 4;
    for (int32_t k = 0; k < np; k++) { probes[k] = (const uint8_t *)argv[4 + k]; lens[k] = (int32_t)strlen(argv[4 + k]); }
    const int64_t co[2] = { 0, n };
    int64_t *adapt = (int64_t *)calloc(KVQ_ADAPT_WORDS, 8);
    int64_t words[KVQ_CLIP_WORDS] = { 0 }, again[KVQ_CLIP_WORDS] = { 0 };
    if (!adapt || kvq_adapt_host_mm(text, n, co, 1, probes, lens, np, per, adapt)) return 4;
    if (kvq_clip_host_mm(text, n, co, 1, probes, lens, np, per, words)) return 4;
    uint8_t *once = (uint8_t *)malloc((size_t)n);
    memcpy(once, text, (size_t)n);
    if (kvq_clip_host_mm(text, n, co, 1, probes, lens, np, per, again)) return 4;
    if (memcmp(once, text, (size_t)n) || memcmp(words, again, sizeof(words))) return 5;      // idempotent, bytes and words
    FILE *o = fopen(argv[2], "wb");
    if (!o || fwrite(text, 1, (size_t)n, o) != (size_t)n || fwrite(adapt, 8, KVQ_ADAPT_WORDS, o) != KVQ_ADAPT_WORDS ||
        fwrite(words, 8, KVQ_CLIP_WORDS, o) != KVQ_CLIP_WORDS) return 6;
    fclose(o);
    free(once); free(adapt); free(text);
    return 0;
}
