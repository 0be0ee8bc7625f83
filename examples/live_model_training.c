/* live_model_training.c -- personal wakeword MODELS on a service's first day, from plain C: streams are connected before anybody has a
 * model, two users train theirs while the batch runs, their slots are connected, and the next audio runs through the new models -- no stream
 * loses its state and no parameter leaves the device (add_wakeword on a running Rustpotter, src/detector.rs:304-346, for a batch of users).
 *   rp_model_bank_new(0 models) -> rp_model_bank_reserve(the largest window and label count ever) -> rp_stream_batch_new_model_bank(every
 *   slot -1) -> rp_stream_batch_set_filters_per_stream(gain normaliser on) -> rp_stream_batch_process ... -> rp_model_bank_train(the users'
 *   recordings) -> rp_stream_batch_set_models(their slots) -> rp_stream_batch_process ...
 * The gain normaliser of a slot works towards the level its user's model was trained at (WakewordModel::rms_level, which the training leaves
 * in the bank) over a window of train_size / 3 chunk levels: both are read from the bank at the start of every call, so a slot connected
 * to a model trained a moment ago is normalised to that model's level from its next chunk on; a slot without a model has gain 1.
 *
 *   gcc -std=c99 -Iinclude examples/live_model_training.c -Lrustpotter_amd -lrustpotter_hip -Wl,-rpath,$PWD/rustpotter_amd -o live_model_training
 *   ./live_model_training tests/golden
 * The directory holds the reference's training recordings (noise0/1/3/4.wav, oye_casa_real_1/3/4/5.wav, oye_casa_g_1/2.wav); user 0 trains
 * on all of them, user 1 on one wakeword recording less; oye_casa_g_1.wav (16 kHz mono i16) is then "spoken" into both users' slots.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rustpotter_hip.h"

static unsigned char *read_file(const char *dir, const char *name, size_t *len) {
    char path[1024];
    snprintf(path, sizeof(path), "%s/%s", dir, name);
    FILE *f = fopen(path, "rb");
    if (!f) { perror(path); return NULL; }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    unsigned char *b = (unsigned char *)malloc(n > 0 ? (size_t)n : 1);
    if (b && n > 0 && fread(b, 1, (size_t)n, f) != (size_t)n) { free(b); b = NULL; }
    fclose(f);
    *len = n > 0 ? (size_t)n : 0;
    return b;
}

enum { SLOTS = 4, FIRST_USER_SLOT = 1, USERS = 2, CHUNK = 480, CALL_CHUNKS = 4, MAX_DET = 4, MAX_WINDOW = 256, MAX_LABELS = 3, FILES = 10 };

/* the recordings and the name each is trained under: the text in brackets is the label, none = "none" */
static const char *const kFiles[FILES] = {"noise0.wav", "noise1.wav", "oye_casa_real_1.wav", "oye_casa_real_3.wav", "oye_casa_real_4.wav",
                                          "oye_casa_real_5.wav", "noise3.wav", "noise4.wav", "oye_casa_g_2.wav", "oye_casa_g_1.wav"};
static const char *const kNames[FILES] = {"noise0.wav", "noise1.wav", "oye_casa_real_1[oye casa].wav", "oye_casa_real_3[oye casa].wav",
                                          "oye_casa_real_4[oye casa].wav", "oye_casa_real_5[oye casa].wav", "noise3.wav", "noise4.wav",
                                          "oye_casa_g_2[oye casa].wav", "oye_casa_g_1[oye casa].wav"};
enum { N_TRAIN = 6, N_TEST = 3, SPOKEN = 9 };

/* `chunks` chunks of 30 ms through the batch, CALL_CHUNKS per call: the users' slots hear `speech` (NULL: silence), the others silence */
static int feed(rp_stream_batch *batch, const int16_t *speech, size_t chunks, int *detections) {
    static int16_t part[SLOTS * CALL_CHUNKS * CHUNK];
    rp_batch_detection det[SLOTS * MAX_DET];
    int32_t n_det[SLOTS], model[SLOTS * MAX_DET], label[SLOTS * MAX_DET];
    float gains[SLOTS * CALL_CHUNKS];
    for (size_t c = 0; c < chunks; c += CALL_CHUNKS) {
        const size_t n = chunks - c < CALL_CHUNKS ? chunks - c : CALL_CHUNKS;
        memset(part, 0, sizeof(part));
        for (int u = 0; speech && u < USERS; ++u)
            memcpy(part + (size_t)(FIRST_USER_SLOT + u) * n * CHUNK, speech + c * CHUNK, n * CHUNK * sizeof(int16_t));
        if (rp_stream_batch_process_multi(batch, part, RP_SAMPLE_I16, n, n * CHUNK, det, model, label, n_det, MAX_DET) < 0 ||
            rp_stream_batch_levels(batch, NULL, gains) < 0) return -1;
        for (int s = 0; s < SLOTS; ++s)
            for (int i = 0; i < n_det[s] && i < MAX_DET; ++i) {
                const rp_batch_detection *d = &det[s * MAX_DET + i];
                printf("slot %d: detection at chunk %d by model %d, label %d, score %.7f, gain of the call's last chunk %.1f\n", s,
                       (int)d->frame / 3 + 1, (int)model[s * MAX_DET + i], (int)label[s * MAX_DET + i], d->score, gains[(size_t)s * n + n - 1]);
                ++*detections;
            }
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s <directory with the golden recordings>\n", argv[0]); return 2; }
    const uint8_t *wavs[FILES];
    size_t wav_lens[FILES];
    memset(wavs, 0, sizeof(wavs));
    int rc = 1, detections = 0;
    rp_ctx *ctx = NULL;
    rp_model_bank *bank = NULL;
    rp_stream_batch *batch = NULL;
    int16_t *speech = NULL;
    for (int i = 0; i < FILES; ++i) {
        wavs[i] = read_file(argv[1], kFiles[i], &wav_lens[i]);
        if (!wavs[i] || wav_lens[i] < 44) { rc = 2; goto out; }
    }
    rp_config cfg;
    rp_config_default(&cfg);
    cfg.detector.min_scores = 1;
    cfg.detector.avg_threshold = 0.f;
    if (rp_ctx_new(0, RP_CTX_HOST_POINTERS, &ctx) < 0) goto out;
    /* 1. an empty bank that declares the largest window and label count it will ever hold: what the batch keeps room for */
    if (rp_model_bank_new(ctx, 0, NULL, 16, NULL, &bank) < 0 || rp_model_bank_reserve(bank, MAX_WINDOW, MAX_LABELS, SLOTS, (size_t)SLOTS * MAX_WINDOW) < 0) goto out;
    /* 2. the live batch: nobody has a model yet */
    const int32_t nobody[SLOTS] = {-1, -1, -1, -1};
    if (rp_stream_batch_new_model_bank(ctx, bank, nobody, &cfg.detector, SLOTS, CALL_CHUNKS, &batch) < 0) goto out;
    /* ... with RustpotterConfig.filters.gain_normalizer, every slot towards the level of ITS model (before the first audio) */
    cfg.filters.gain_normalizer.enabled = true;
    cfg.filters.gain_normalizer.min_gain = 0.5f;
    cfg.filters.gain_normalizer.max_gain = 2.0f;
    if (rp_stream_batch_set_filters_per_stream(batch, &cfg.filters) < 0) goto out;
    if (feed(batch, NULL, 20, &detections) < 0) goto out;
    printf("%d model(s) in the bank, %d detection(s) so far\n", rp_model_bank_size(bank), detections);
    /* 3. two users train while the batch runs: user 0 on every recording, user 1 on one wakeword recording less; both are tested on the
     *    same three.  The trained parameters go from the training workspace straight into bank slots 0 and 1. */
    const char *train_names[2 * N_TRAIN], *test_names[2 * N_TEST];
    const uint8_t *train_wavs[2 * N_TRAIN], *test_wavs[2 * N_TEST];
    size_t train_lens[2 * N_TRAIN], test_lens[2 * N_TEST], train_counts[USERS] = {N_TRAIN, N_TRAIN - 1}, test_counts[USERS] = {N_TEST, N_TEST};
    size_t nt = 0, ne = 0;
    for (int u = 0; u < USERS; ++u) {
        for (size_t i = 0; i < train_counts[u]; ++i, ++nt) { train_names[nt] = kNames[i]; train_wavs[nt] = wavs[i]; train_lens[nt] = wav_lens[i]; }
        for (int i = 0; i < N_TEST; ++i, ++ne) { test_names[ne] = kNames[N_TRAIN + i]; test_wavs[ne] = wavs[N_TRAIN + i]; test_lens[ne] = wav_lens[N_TRAIN + i]; }
    }
    rp_train_options opt;
    memset(&opt, 0, sizeof(opt));
    opt.m_type = RP_MODEL_TINY; opt.learning_rate = 0.027f; opt.epochs = 100; opt.mfcc_size = 16; opt.seed = 7;
    float loss[USERS], accuracy[USERS];
    if (rp_model_bank_train(bank, 0, USERS, &opt, NULL, train_counts, train_names, train_wavs, train_lens, test_counts, test_names, test_wavs,
                            test_lens, NULL, NULL, NULL, NULL, loss, accuracy) < 0) goto out;
    for (int u = 0; u < USERS; ++u)
        printf("trained model %d: windows of %d frames, %d labels, loss %.5f, test accuracy %.2f, rms level %.4f\n", u,
               rp_model_bank_train_size(bank, u), rp_model_bank_labels(bank, u), loss[u], accuracy[u], rp_model_bank_rms_level(bank, u));
    /* 4. their slots are connected (and reset, as add_wakeword does) */
    const int32_t theirs[USERS] = {0, 1};
    if (rp_stream_batch_set_models(batch, FIRST_USER_SLOT, USERS, theirs) < 0) goto out;
    /* 5. they speak: one second of silence, a recording in whole chunks (canonical 44-byte RIFF header), three seconds of silence */
    const size_t pad = 34, rec = (wav_lens[SPOKEN] - 44) / 2 / CHUNK, total = pad + rec + 3 * pad;
    speech = (int16_t *)calloc(total * CHUNK, sizeof(int16_t));
    if (!speech) goto out;
    memcpy(speech + pad * CHUNK, wavs[SPOKEN] + 44, rec * CHUNK * sizeof(int16_t));
    if (feed(batch, speech, total, &detections) < 0) goto out;
    printf("%d model(s) in the bank, %d detection(s), %d pool growth(s)\n", rp_model_bank_size(bank), detections, rp_model_bank_pool_growths(bank));
    rc = 0;
out:
    if (rc == 1) fprintf(stderr, "error: %s\n", rp_last_error());
    free(speech);
    rp_stream_batch_free(batch);   /* the batch borrows the bank and the context: a batch is freed before its bank */
    rp_model_bank_free(bank);
    rp_ctx_free(ctx);
    for (int i = 0; i < FILES; ++i) free((void *)wavs[i]);
    return rc;
}
