// ingest_mail_main.cpp — csrc/ingest_mail.h on the CPU: the word format of the scalar mailbox and the host's way of taking it.
// usage: ingest_mail_test <case>; exit status 0 when every check of the case held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../bsc-nav_amd/csrc/ingest_mail.h"

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

enum { N = 18 };
static const int64_t UNTOUCHED = 0x5a5a5a5a5a5a5a5all;
static const int64_t BIG = (1ll << 47) - 1;

static void post(volatile int64_t *mb, const int64_t *v, uint64_t seq)
{
    for (int k = 0; k < N; ++k) mb[k] = mail_encode(v[k], seq);
}

static void case_all_tagged()
{
    volatile int64_t mb[N];
    int64_t v[N], out[N];
    for (int k = 0; k < N; ++k) { v[k] = 1000 * k + 7; out[k] = UNTOUCHED; }
    post(mb, v, 5);
    CHECK(mail_take(mb, N, 5, out));
    for (int k = 0; k < N; ++k) CHECK(out[k] == v[k] && mail_tagged(mb[k], 5) && !mail_tagged(mb[k], 6));
    int64_t big[MAIL_MAX_WORDS + 1];
    CHECK(!mail_take(mb, MAIL_MAX_WORDS + 1, 5, big));       // more words than the copy holds: refused before any read
}

static void case_one_stale_word()
{
    for (int stale = 0; stale < N; ++stale) {
        volatile int64_t mb[N];
        int64_t v[N], out[N];
        for (int k = 0; k < N; ++k) { v[k] = k; out[k] = UNTOUCHED; }
        post(mb, v, 8);
        mb[stale] = mail_encode(v[stale], 7);               // the previous call's word has not been overwritten yet
        CHECK(!mail_take(mb, N, 8, out));
        for (int k = 0; k < N; ++k) CHECK(out[k] == UNTOUCHED);
        mb[stale] = mail_encode(v[stale], 8);
        CHECK(mail_take(mb, N, 8, out) && out[stale] == v[stale]);
    }
}

static void case_sign_and_range()
{
    volatile int64_t mb[N];
    int64_t v[N] = {-1, -5, BIG, -BIG, 0, 1, -(1ll << 40), 1ll << 40}, out[N];
    const uint64_t seqs[] = {1ull, 0x7fffull, 0xffffull, 0x123456789abcull};
    for (uint64_t seq : seqs) {
        post(mb, v, seq);
        memset(out, 0x11, sizeof out);
        CHECK(mail_take(mb, N, seq, out));
        for (int k = 0; k < N; ++k) CHECK(out[k] == v[k]);
    }
}

static void case_tag_wraps()
{
    volatile int64_t mb[N];
    int64_t v[N], w[N], out[N];
    for (int k = 0; k < N; ++k) { v[k] = k + 1; w[k] = -(k + 1); out[k] = UNTOUCHED; }
    post(mb, v, 0xffff);
    CHECK(mail_take(mb, N, 0xffff, out) && out[N - 1] == N);
    CHECK(!mail_take(mb, N, 0x10000, out) && out[0] == 1);   // the next call (tag 0) has not written yet
    post(mb, w, 0x10000);
    CHECK(mail_tag(0x10000) == 0 && (mb[0] & 0xffff) == 0);
    CHECK(mail_take(mb, N, 0x10000, out));
    for (int k = 0; k < N; ++k) CHECK(out[k] == w[k]);
    CHECK(!mail_take(mb, N, 0xffff, out));
}

// a word rewritten between two takes: each take is consistent in itself — the value it returns belongs to the tag it checked
static void case_rewrite_between_takes()
{
    volatile int64_t mb[N];
    int64_t v[N], out[N];
    for (int k = 0; k < N; ++k) { v[k] = 100 + k; out[k] = UNTOUCHED; }
    post(mb, v, 3);
    CHECK(mail_take(mb, N, 3, out) && out[4] == 104);
    mb[4] = mail_encode(999, 4);                             // the next call's store lands in one word
    int64_t again[N];
    for (int k = 0; k < N; ++k) again[k] = UNTOUCHED;
    CHECK(!mail_take(mb, N, 3, again));                      // call 3 no longer holds the whole mailbox: nothing of call 4 leaks out
    for (int k = 0; k < N; ++k) CHECK(again[k] == UNTOUCHED);
    CHECK(!mail_take(mb, N, 4, again) && again[4] == UNTOUCHED);
    for (int k = 0; k < N; ++k) mb[k] = mail_encode(k == 4 ? 999 : 2 * v[k], 4);
    CHECK(mail_take(mb, N, 4, again));
    for (int k = 0; k < N; ++k) CHECK(again[k] == (k == 4 ? 999 : 2 * v[k]));
    CHECK(out[4] == 104);                                    // what the first take returned was call 3's, untouched since
}

int main(int argc, char **argv)
{
    const struct { const char *name; void (*fn)(); } cases[] = {
        {"all_tagged", case_all_tagged}, {"one_stale_word", case_one_stale_word}, {"sign_and_range", case_sign_and_range},
        {"tag_wraps", case_tag_wraps}, {"rewrite_between_takes", case_rewrite_between_takes}};
    for (const auto &c : cases)
        if (argc == 2 && !strcmp(argv[1], c.name)) { c.fn(); printf("ok %s\n", c.name); return 0; }
    fprintf(stderr, "usage: ingest_mail_test <case>\n");
    return 2;
}
