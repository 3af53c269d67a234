// aisx_track.cpp -- aisx_track_* (include/aisx.h): the vessel table on the host, plain C++, one row after the other.
// It is the specification of the device form (k_track.h, aisx_track.hip), which must equal it array for array.
//
// Values are kept as transmitted: the protocol's own "not available" codes (longitude 181 degrees, speed 1023 ...) are
// values like any other and overwrite what was known.  Mapping them is out of scope here.
#include <string.h>

#include <unordered_map>
#include <vector>

#include "../../include/aisx.h"
#include "k_track.h"

using namespace aisx;

static_assert(TRK_NCOL == AISX_TRK_NCOL && TC_COUNT == AISX_TRK_COL_COUNT && TC_CHAN == AISX_TRK_COL_CHAN, "column order");
static_assert(TRK_NCNT == AISX_TRK_NCNT && TN_BAD == AISX_TRK_CNT_BAD_INPUT && TN_REMOVED == AISX_TRK_CNT_REMOVED, "count order");

struct aisx_track {
    int capacity = 0;
    std::vector<int32_t> cols; // [TRK_NCOL][capacity]
    std::vector<char> strs;    // [capacity][MSG_STR]
    std::vector<int> changed;
    std::unordered_map<int32_t, int> index; // MMSI -> vessel
    int count[TRK_NCNT] = {};
};

extern "C" int aisx_track_create(aisx_track** out, int capacity)
{
    if (!out || capacity < 1 || capacity > TRK_MAX)
        return AISX_ERR_INVALID;
    aisx_track* h = new aisx_track();
    h->capacity = capacity;
    h->cols.assign((size_t)TRK_NCOL * capacity, MSG_NA);
    h->strs.assign((size_t)MSG_STR * capacity, 0);
    *out = h;
    return AISX_OK;
}

extern "C" int aisx_track_destroy(aisx_track* h)
{
    delete h;
    return AISX_OK;
}

extern "C" int aisx_track_update(aisx_track* h, const int32_t* cols, long col_stride, const char* strs, const aisx_pdu* recs, int n,
                                 int32_t stamp, int* counts)
{
    if (!h || n < 0 || col_stride < n || (n > 0 && (!cols || !strs)))
        return AISX_ERR_INVALID;
    const size_t cap = (size_t)h->capacity;
    int merged = 0, skipped = 0, dropped = 0;
    h->changed.clear();
    std::vector<char> touched; // by vessel, this call
    for (int i = 0; i < n; i++) {
        const int32_t mmsi = cols[(size_t)MC_MMSI * col_stride + i];
        if ((cols[(size_t)MC_FLAGS * col_stride + i] & MSG_FL_BAD_RECORD) || mmsi == MSG_NA) {
            skipped++;
            continue;
        }
        int v;
        const auto it = h->index.find(mmsi);
        if (it != h->index.end())
            v = it->second;
        else if (h->count[TN_VESSELS] == h->capacity) {
            dropped++;
            continue;
        } else {
            v = h->count[TN_VESSELS]++;
            h->index.emplace(mmsi, v);
            for (int c = 0; c < TRK_NCOL; c++)
                h->cols[c * cap + v] = c == TC_COUNT ? 0 : MSG_NA;
            memset(&h->strs[(size_t)v * MSG_STR], 0, MSG_STR);
        }
        for (int c = 0; c < MSG_NCOL; c++) {
            const int32_t x = cols[(size_t)c * col_stride + i];
            if (x != MSG_NA || trk_always(c))
                h->cols[c * cap + v] = x;
        }
        const char* s = strs + (size_t)i * MSG_STR;
        for (int k = 0; k < 3; k++)
            if (s[4 * trk_slot_word(k)] != 0)
                memcpy(&h->strs[(size_t)v * MSG_STR + 4 * trk_slot_word(k)], s + 4 * trk_slot_word(k), 4 * (size_t)trk_slot_words(k));
        int32_t& cnt = h->cols[TC_COUNT * cap + v];
        if (cnt < INT32_MAX)
            cnt++;
        h->cols[TC_STAMP * cap + v] = stamp;
        if (cols[(size_t)MC_LON * col_stride + i] != MSG_NA && cols[(size_t)MC_LAT * col_stride + i] != MSG_NA)
            h->cols[TC_POS_STAMP * cap + v] = stamp;
        h->cols[TC_CHAN * cap + v] = recs ? recs[i].chan : MSG_NA;
        merged++;
        if (touched.size() <= (size_t)v)
            touched.resize((size_t)h->count[TN_VESSELS], 0);
        if (!touched[v]) {
            touched[v] = 1;
            h->changed.push_back(v);
        }
    }
    h->count[TN_MERGED] = merged;
    h->count[TN_SKIPPED] = skipped;
    h->count[TN_DROPPED] = dropped;
    h->count[TN_CHANGED] = (int)h->changed.size();
    h->count[TN_FULL] = dropped > 0;
    if (counts)
        memcpy(counts, h->count, sizeof h->count);
    return AISX_OK;
}

extern "C" int aisx_track_expire(aisx_track* h, int32_t min_stamp, int* counts)
{
    if (!h)
        return AISX_ERR_INVALID;
    const size_t cap = (size_t)h->capacity;
    const int nv = h->count[TN_VESSELS];
    int d = 0;
    h->index.clear();
    for (int v = 0; v < nv; v++) {
        if (h->cols[TC_STAMP * cap + v] < min_stamp)
            continue;
        if (d != v) {
            for (int c = 0; c < TRK_NCOL; c++)
                h->cols[c * cap + d] = h->cols[c * cap + v];
            memcpy(&h->strs[(size_t)d * MSG_STR], &h->strs[(size_t)v * MSG_STR], MSG_STR);
        }
        h->index.emplace(h->cols[MC_MMSI * cap + d], d);
        d++;
    }
    h->changed.clear();
    h->count[TN_VESSELS] = d;
    h->count[TN_REMOVED] = nv - d;
    h->count[TN_CHANGED] = 0;
    if (counts)
        memcpy(counts, h->count, sizeof h->count);
    return AISX_OK;
}

extern "C" int aisx_track_data(const aisx_track* h, const int32_t** cols, long* col_stride, const char** strs, int* nvessels)
{
    if (!h)
        return AISX_ERR_INVALID;
    if (cols)
        *cols = h->cols.data();
    if (col_stride)
        *col_stride = h->capacity;
    if (strs)
        *strs = h->strs.data();
    if (nvessels)
        *nvessels = h->count[TN_VESSELS];
    return AISX_OK;
}

extern "C" int aisx_track_changed(const aisx_track* h, const int** idx, int* nchanged)
{
    if (!h)
        return AISX_ERR_INVALID;
    if (idx)
        *idx = h->changed.data();
    if (nchanged)
        *nchanged = (int)h->changed.size();
    return AISX_OK;
}
