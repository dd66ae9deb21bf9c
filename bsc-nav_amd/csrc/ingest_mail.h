// ingest_mail.h — the word format of the scalar mailbox between k_block_totals (ingest.hip) and the host (read_batch_counts).
// Host-only: plain C++, no HIP include.  The device writes every scalar of the call as ONE 8-byte word `value << 16 | seq & 0xffff`
// with a relaxed system-scope store (mail_encode is constexpr, so the kernel calls this very function); the scalars are counts
// below 2^47, so the value survives the shift, and the host takes the mailbox once every word carries the tag of the call,
// whatever order the fabric delivered the words in.
#pragma once
#include <stdint.h>

#define MAIL_TAG_BITS 16
#define MAIL_MAX_WORDS 32       // mail_take copies the mailbox to its stack

constexpr uint64_t mail_tag(uint64_t seq) { return seq & ((1ull << MAIL_TAG_BITS) - 1ull); }
constexpr int64_t mail_encode(int64_t value, uint64_t seq) { return (int64_t)(((uint64_t)value << MAIL_TAG_BITS) | mail_tag(seq)); }
constexpr bool mail_tagged(int64_t word, uint64_t seq) { return mail_tag((uint64_t)word) == mail_tag(seq); }

// The n <= MAIL_MAX_WORDS words of the mailbox, if all of them belong to call `seq`: every word is loaded ONCE (acquire) and both
// the tag check and the value (arithmetic shift: a value in +-2^47 keeps its sign) come from that copy, so a word the device
// rewrites meanwhile cannot pass the check with one call's tag and deliver another call's value.  false: not yet — out is untouched.
static inline bool mail_take(const volatile int64_t *mb, int n, uint64_t seq, int64_t *out)
{
    int64_t w[MAIL_MAX_WORDS];
    if (n > MAIL_MAX_WORDS) return false;
    for (int k = 0; k < n; ++k) {
        w[k] = __atomic_load_n(&mb[k], __ATOMIC_ACQUIRE);
        if (!mail_tagged(w[k], seq)) return false;
    }
    for (int k = 0; k < n; ++k) out[k] = w[k] >> MAIL_TAG_BITS;
    return true;
}
