/* Host driver of the packer (lpcnet_amd/csrc/model_pack.c, compiled into this program): reads a weight blob, packs the four-stream image and the
 * two-group kernel's, and prints per wave of the two-group image what the kernel derives its slot plan from (lpcnet_amd/csrc/slot_plan.h): the slot
 * bounds, the head length, and per slot whether it has rows and candidate rows.  The packer itself prints its slot -> wave maps on stderr under
 * LPCN_DEAL_PRINT=1 and says so when it ignores a forced map (LPCN_DEAL_FORCE / LPCN_DEAL_FORCE_X2).   deal_print_host <blob file> */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../lpcnet_amd/csrc/model_pack.c"

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    long len = ftell(f);
    fseek(f, 0, SEEK_SET);
    unsigned char *blob = (unsigned char *)malloc((size_t)len);
    if (fread(blob, 1, (size_t)len, f) != (size_t)len) return 2;
    fclose(f);
    static lpcn_model_host m, x;
    if (lpcn_model_parse(&m, blob, (int)len) != 0) { printf("parse failed\n"); return 1; }
    const int have = lpcn_model_pack_x2(&m, &x) == 0;
    printf("x2 %d nw %d\n", have, have ? x.nw : 0);
    if (have) {
        for (int w = 0; w < LPCN_WAVES; w++) {
            int live = 0, cand = 0;
            for (int k = 0; k < LPCN_MAX_SLOTS; k++)
                for (int lane = 0; lane < 64; lane++) {
                    const int r = x.pk_a_row[(w * LPCN_MAX_SLOTS + k) * 64 + lane];
                    if (r >= 0) live |= 1 << k;
                    if (r >= 2 * LPCN_N_A) cand |= 1 << k;
                }
            printf("wave %d bounds %d %d %d %d head %d live %d cand %d\n", w, x.pk_a_bound[w][0], x.pk_a_bound[w][1], x.pk_a_bound[w][2], x.pk_a_bound[w][3],
                   x.pk_a_head[w], live, cand);
        }
    }
    return 0;
}
