/* parse_tables.c -- the tables of the AAC parsers (parse_core.h), built once on the host; the device gets a copy, so
 * that dequantisation is a look-up times the scalefactor wherever it runs and nothing of it is computed on the device:
 *   lut / node   the code trees of parse_bits.h (book 0 = scalefactors, 1..11 = the spectral books)
 *   pow2sf       ff_aac_pow2sf_tab: 2^((i - 200) / 4) (aac_tablegen.h)
 *   mag          q^(4/3), q < 16 (aactab.c: codebook vector values)
 *   esc          cbrtf((float)q) * (float)q, q < 8192: every value an escape sequence of at most 8 ones can carry
 *   band tables, aac_tns_map
 */
#include <math.h>
#include <pthread.h>
#include <string.h>
#include "aac_iso_tables.h"
#include "parse_bits.h"
#include "parse_core.h"

static HeaacParseTables g_pt;
static int g_pt_bad;
static pthread_once_t g_pt_once = PTHREAD_ONCE_INIT;

static void put_tree(int book, const Tree *t)
{
    if (t->count > HEAAC_PT_NODES) { g_pt_bad = 1; return; }
    memcpy(g_pt.lut[book], t->lut, sizeof(g_pt.lut[book]));
    for (int k = 0; k < t->count; k++) {
        g_pt.node[book][k][0] = t->n[k].child[0];
        g_pt.node[book][k][1] = t->n[k].child[1];
    }
}

static void pt_init(void)
{
    static Tree t;                                     /* 6 KB: not on the stack of whoever calls first */
    g_pt_bad |= tree_build(&t, aac_sf_code, NULL, aac_sf_bits, 121);
    put_tree(0, &t);
    for (int b = 0; b < 11; b++) {
        g_pt_bad |= tree_build(&t, NULL, aac_spec_code + aac_spec_first[b], aac_spec_bits + aac_spec_first[b],
                               aac_spec_first[b + 1] - aac_spec_first[b]);
        put_tree(b + 1, &t);
    }
    for (int i = 0; i < 428; i++) g_pt.pow2sf[i] = (float)pow(2, (i - 200) / 4.);
    for (int q = 0; q < 16; q++) g_pt.mag[q] = (float)pow((double)q, 4.0 / 3.0);
    for (int q = 0; q < 8192; q++) g_pt.esc[q] = cbrtf((float)q) * (float)q;
    memcpy(g_pt.num_swb_1024, aac_num_swb_1024, 13);
    memcpy(g_pt.num_swb_128, aac_num_swb_128, 13);
    memcpy(g_pt.pred_sfb_max, aac_pred_sfb_max, 13);
    memcpy(g_pt.tns_max_bands_1024, aac_tns_max_bands_1024, 13);
    memcpy(g_pt.tns_max_bands_128, aac_tns_max_bands_128, 13);
    memcpy(g_pt.swb_first_1024, aac_swb_first_1024, sizeof(aac_swb_first_1024));
    memcpy(g_pt.swb_first_128, aac_swb_first_128, sizeof(aac_swb_first_128));
    memcpy(g_pt.swb_offset_1024, aac_swb_offset_1024, sizeof(aac_swb_offset_1024));
    memcpy(g_pt.swb_offset_128, aac_swb_offset_128, sizeof(aac_swb_offset_128));
    memcpy(g_pt.tns_map, aac_tns_map, sizeof(aac_tns_map));
}

/* The one host copy (NULL if a code book did not fit its tree: never with the shipped tables). */
const HeaacParseTables *heaac_parse_tables(void)
{
    pthread_once(&g_pt_once, pt_init);
    return g_pt_bad ? NULL : &g_pt;
}

uint64_t heaac_aac_tables_fingerprint(void)
{
    uint64_t h = 1469598103934665603ull;
#define MIX(arr) do { const uint8_t *p_ = (const uint8_t *)(arr); for (size_t i_ = 0; i_ < sizeof(arr); i_++) { h ^= p_[i_]; h *= 1099511628211ull; } } while (0)
    MIX(aac_sf_code); MIX(aac_sf_bits); MIX(aac_spec_first); MIX(aac_spec_code); MIX(aac_spec_bits);
    MIX(aac_num_swb_1024); MIX(aac_num_swb_128); MIX(aac_pred_sfb_max); MIX(aac_tns_max_bands_1024);
    MIX(aac_tns_max_bands_128); MIX(aac_swb_offset_1024); MIX(aac_swb_offset_128); MIX(aac_tns_map);
#undef MIX
    return h;
}
