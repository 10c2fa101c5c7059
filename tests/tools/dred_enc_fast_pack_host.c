/* Host driver of the FAST packer (lpcnet_amd/csrc/dred_fast_pack.h) on a blob's DRED ENCODER, with the loader compiled in
 * (lpcnet_amd/csrc/model_pack.c): reads a weight blob, packs the three GRU input matrices of its encoder (enc_dense2 / 4 / 6) and writes, per GRU, the
 * header {n_in, n, tiles, blocks}, start [3 tiles + 1], pos [blocks] (int32) and the image read back as the dense matrix [3 n][n_in] (float32) to
 * the output file -- the format of dred_fast_pack_host.c, the decoder's driver.  The last line on stdout is "ok".
 *     dred_enc_fast_pack_host <blob file> <output file> */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../lpcnet_amd/csrc/model_pack.c"
#include "../../lpcnet_amd/csrc/dred_fast_pack.h"

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    long len = ftell(f);
    fseek(f, 0, SEEK_SET);
    unsigned char *blob = (unsigned char *)malloc((size_t)len);
    if (fread(blob, 1, (size_t)len, f) != (size_t)len) return 2;
    fclose(f);
    static lpcn_model_host m;
    if (lpcn_model_parse(&m, blob, (int)len) != 0 || m.dred_enc.present != 1) { printf("no float encoder\n"); return 1; }
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    for (int g = 0; g < 3; g++) {
        const lpcn_gru_layer *G = &m.dred_enc.gru[g];
        lpcn_dred_fast_gru pk;
        const int rc = lpcn_dred_fast_pack(G->w, G->idx, G->n_in, G->n, &pk);
        if (rc) { printf("pack of GRU %d failed: %d\n", g, rc); return 1; }
        const int blocks = pk.start[3 * pk.tiles], head[4] = {pk.n_in, pk.n, pk.tiles, blocks};
        float *dense = (float *)malloc(sizeof(float) * 3 * (size_t)pk.n * pk.n_in);
        if (!dense) return 2;
        lpcn_dred_fast_unpack(&pk, dense);
        fwrite(head, sizeof(int), 4, o);
        fwrite(pk.start, sizeof(int), 3 * (size_t)pk.tiles + 1, o);
        fwrite(pk.pos, sizeof(int), (size_t)blocks, o);
        fwrite(dense, sizeof(float), 3 * (size_t)pk.n * pk.n_in, o);
        printf("gru %d: %d inputs, %d units, %d tiles, %d union blocks of %d\n", g, pk.n_in, pk.n, pk.tiles, blocks, G->nb);
        free(dense);
        lpcn_dred_fast_release(&pk);
    }
    fclose(o);
    free(blob);
    printf("ok\n");
    return 0;
}
