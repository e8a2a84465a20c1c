/* sbr_parse_tables.c -- the code books of the payload walk of sbr_core.h: the ten SBR and the ten PS books of
 * sbr_iso_tables.h as one flat table of tree nodes, built on the host with parse_bits.h's tree_build (the trees
 * sbr_parse.c reads with) and uploaded once per device context next to the tables of parse_core.h. */
#include <pthread.h>
#include <string.h>
#include "sbr_iso_tables.h"
#include "parse_bits.h"
#include "sbr_core.h"

static HeaacSbrParseTables g_st;
static int g_st_bad;
static pthread_once_t g_st_once = PTHREAD_ONCE_INIT;

static void st_init(void)
{
    static Tree t;                                     /* 6 KB: not on the stack of whoever calls first */
    int total = 0;
    for (int k = 0; k < HEAAC_ST_BOOKS; k++) {
        const int ps = k >= 10, j = k % 10;
        const uint16_t *first = ps ? ps_huff_first : sbr_huff_first;
        g_st_bad |= tree_build(&t, (ps ? ps_huff_code : sbr_huff_code) + first[j], NULL,
                               (ps ? ps_huff_bits : sbr_huff_bits) + first[j], first[j + 1] - first[j]);
        if (total + t.count > HEAAC_ST_NODES) { g_st_bad = 1; return; }
        g_st.root[k] = (uint16_t)total;
        g_st.bias[k] = ps ? ps_huff_offset[j] : sbr_huff_lav[j];
        for (int i = 0; i < t.count; i++) {
            g_st.node[total + i][0] = t.n[i].child[0];
            g_st.node[total + i][1] = t.n[i].child[1];
        }
        total += t.count;
    }
}

/* The one host copy (NULL if a code book did not fit: never with the shipped tables). */
const HeaacSbrParseTables *heaac_sbr_parse_tables(void)
{
    pthread_once(&g_st_once, st_init);
    (void)bits_init;                                   /* parse_bits.h's non-inline static, unused here: no warning */
    return g_st_bad ? NULL : &g_st;
}
