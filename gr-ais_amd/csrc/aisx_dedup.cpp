// aisx_dedup.cpp -- aisx_dedup_* (include/aisx.h): PDUs heard by several receivers, suppressed on the host, plain C++, one
// record after the other.  It is the specification of the device form (k_dedup.h, aisx_dedup.hip), which must equal it
// array for array.
#include <string.h>

#include <unordered_map>

#include "../../include/aisx.h"
#include "k_dedup.h"

using namespace aisx;

static_assert(DD_NCNT == AISX_DEDUP_NCNT && DN_KEPT == AISX_DEDUP_CNT_KEPT && DN_DUP_CALL == AISX_DEDUP_CNT_DUP_CALL &&
                  DN_DUP_WINDOW == AISX_DEDUP_CNT_DUP_WINDOW && DN_BAD_LEN == AISX_DEDUP_CNT_BAD_LEN,
              "count order");

struct aisx_dedup {
    int window = 0, length_max = 0;
    std::unordered_map<uint64_t, long long> kept; // key -> the stamp of the call that kept it last
    bool have_prev = false;
    long long prev = 0;
};

extern "C" int aisx_dedup_key(const uint8_t* pdu, int len, uint64_t* key)
{
    if (!key || len < 0 || (len > 0 && !pdu))
        return AISX_ERR_INVALID;
    *key = dd_key(pdu, len);
    return AISX_OK;
}

extern "C" int aisx_dedup_create(aisx_dedup** out, int window, int length_max)
{
    if (!out)
        return AISX_ERR_INVALID;
    *out = nullptr;
    if (window < 0 || window > DD_MAX_WINDOW || length_max < 2 || length_max > 1024)
        return AISX_ERR_INVALID;
    aisx_dedup* h = new aisx_dedup();
    h->window = window;
    h->length_max = length_max;
    *out = h;
    return AISX_OK;
}

extern "C" int aisx_dedup_destroy(aisx_dedup* h)
{
    delete h;
    return AISX_OK;
}

extern "C" int aisx_dedup_reset(aisx_dedup* h)
{
    if (!h)
        return AISX_ERR_INVALID;
    h->kept.clear();
    h->have_prev = false;
    return AISX_OK;
}

extern "C" int aisx_dedup_update(aisx_dedup* h, const aisx_pdu* pdus, const uint8_t* bytes, int n, const int32_t* marks,
                                 int32_t stamp, aisx_pdu* out_pdus, int32_t* first, int32_t* copies, int32_t* out_marks,
                                 int* counts)
{
    if (!h || n < 0 || (n > 0 && !pdus))
        return AISX_ERR_INVALID;
    const long long now = stamp;
    if (h->have_prev && now <= h->prev)
        return AISX_ERR_OUT_OF_RANGE;
    h->have_prev = true;
    h->prev = now;
    for (auto it = h->kept.begin(); it != h->kept.end();) // what has left the window for good
        it = it->second < now - h->window ? h->kept.erase(it) : ++it;
    int cnt[DD_NCNT] = {};
    cnt[DN_IN] = n;
    std::unordered_map<uint64_t, int> here; // key -> output record, this call
    int j = 0;
    auto keep = [&](int i) {
        if (out_pdus)
            out_pdus[j] = pdus[i];
        if (marks && out_marks)
            out_marks[j] = marks[i];
        if (copies)
            copies[j] = 1;
        if (first)
            first[i] = j;
        return j++;
    };
    for (int i = 0; i < n; i++) {
        const int len = pdus[i].len;
        if (len < 0 || len > h->length_max - 1) {
            cnt[DN_BAD_LEN]++;
            keep(i);
            continue;
        }
        const uint64_t key = dd_key(bytes + pdus[i].offset, len);
        const auto was = h->kept.find(key);
        if (was != h->kept.end() && was->second < now) { // (its stamp is at least now - window: older ones are gone)
            cnt[DN_DUP_WINDOW]++;
            if (first)
                first[i] = (int32_t)(-1 - (now - was->second));
            continue;
        }
        const auto dup = here.find(key);
        if (dup != here.end()) {
            cnt[DN_DUP_CALL]++;
            if (first)
                first[i] = dup->second;
            if (copies)
                copies[dup->second]++;
            continue;
        }
        here.emplace(key, keep(i));
        h->kept[key] = now;
    }
    cnt[DN_KEPT] = j;
    if (counts)
        memcpy(counts, cnt, sizeof cnt);
    return AISX_OK;
}
