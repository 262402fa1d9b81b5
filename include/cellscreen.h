/*
 * cellscreen.h -- C ABI of libcellscreen.so, the MI355X (gfx950) cell-crop
 * anomaly-screening path.
 *
 * The reference (Kmatsuo57/cell-image-analysis) is two Python classes with no
 * FFI; what this library replaces, entry point by entry point:
 *
 *   cs_model_load / cs_model_from_arrays
 *        ProductionMutantScreening.load_trained_models    improved_detection.py:23-46
 *        (the StarDist fetch at :44 is cell extraction, out of scope)
 *   cs_screen
 *        ProductionMutantScreening.compute_anomaly_scores improved_detection.py:117-153
 *        = autoencoder.predict (:125) + per-cell MSE/MAE (:126-127) + encoder.predict
 *          (:130-131) + scaler.transform (:134) + pca.transform (:135) + 2x OneClassSVM
 *          predict / decision_function (:138-142) + score negation (:149-150)
 *   cs_reconstruct
 *        evaluate_reconstruction_quality numerics   CAE_improved_modeltrain.py:335-339
 *   cs_encode
 *        encoder.predict + flatten      improved_detection.py:130-131, CAE...:401-402
 *   cs_layer_output, cs_scaler_pca, cs_svm_decision
 *        stage-level taps used by the parity tests (oracle inputs to each stage)
 *   cs_preprocess
 *        equalize_adapthist + resize of each crop   improved_detection.py:98-99, CAE...:92-93
 *   cs_extract_measure / cs_extract_fill
 *        the quality-cell extraction that follows segmentation: regionprops + the border / area /
 *        eccentricity / intensity rules + the bbox crop + the preprocess above
 *                                   improved_detection.py:61-111, CAE_improved_modeltrain.py:54-107
 *        (the StarDist segmentation itself, :59-60 / :52-53, stays with the caller)
 *   cs_segment_threshold / cs_segment_split / cs_segment_split_intensity
 *        the library's own classical segmenter (no reference counterpart, and no StarDist): Otsu or
 *        fixed threshold, optional hole filling, connected-component labels for the extraction above
 *        (cs_segment_smooth, cs_segment_background, cs_segment_local, cs_segment_hysteresis, cs_segment_noise,
 *        cs_segment_clean: optional stages before the labels)
 *   cs_label_match
 *        scores a label image against ground truth: object matching by intersection over union, the
 *        rule of StarDist's `matching` made unique (no reference counterpart)
 *   cs_label_expand
 *        grows the objects of a label image outwards by a fixed distance, halfway to their neighbours at
 *        most: skimage.segmentation.expand_labels between a nuclear segmentation and the extraction
 *        (no reference counterpart)
 *   cs_image_quality / cs_object_focus
 *        whether an image, a mesh tile of it or an object is worth measuring: intensity, extreme and saturation counts and
 *        the sums behind the Laplacian variance, Tenengrad and Brenner focus measures, as exact integers (CellProfiler's
 *        MeasureImageQuality: FocusScore, LocalFocusScore, PercentMinimal / PercentMaximal; no reference counterpart)
 *   cs_illum_tile_stats / cs_illum_reduce / cs_illum_apply
 *        flat-field correction from a plate's own images: one multiplicative illumination function per channel on a
 *        tile mesh, estimated across all fields and divided out of every field, in integers (CellProfiler's
 *        CorrectIlluminationCalculate / CorrectIlluminationApply; no reference counterpart)
 *   cs_spot_detect / cs_spot_fill
 *        puncta in one channel and how many of them every object holds: the local maxima of a difference-of-Gaussians
 *        response, computed in integers, as a list sorted by image and raster order and as per-object records
 *        (skimage.feature.blob_dog / peak_local_max, TrackMate's DoG detector, CellProfiler's IdentifyPrimaryObjects +
 *        RelateObjects on speckles; no reference counterpart)
 *   cs_label_intensity
 *        measures every object of a label image in every channel: area, centroid, integrated / mean / std /
 *        min / max intensity and the intensity-weighted centroid, as exact integer sums
 *        (skimage.measure.regionprops with an intensity image, scipy.ndimage's labelled statistics,
 *        CellProfiler's MeasureObjectIntensity; no reference counterpart)
 *   cs_label_quantiles
 *        the robust half of the same measurement: per object and channel the median, any quantiles and the
 *        median absolute deviation, as exact integer order statistics (scipy.ndimage.median, numpy.quantile
 *        per object, CellProfiler's MedianIntensity / MADIntensity / quartiles; no reference counterpart)
 *   cs_label_texture
 *        the texture of the same objects: per object, channel and direction the grey-level co-occurrence
 *        matrix, reduced to the exact records Haralick's 13 features follow from (mahotas.features.haralick,
 *        skimage's graycomatrix / graycoprops, CellProfiler's MeasureTexture; no reference counterpart)
 *   cs_label_shape
 *        the size and shape of the same objects: ten moments, the bounding box, the 2 x 2 bit quads, the perimeter
 *        classes and the convex hull's records as exact integers, from which area, axes, orientation, Hu moments,
 *        perimeter, form factor, Euler number, solidity and Feret diameters follow (skimage.measure.regionprops'
 *        geometry properties, CellProfiler's MeasureObjectSizeShape; no reference counterpart)
 *   cs_label_neighbors / cs_label_neighbors_pairs
 *        the neighbourhood of the same objects: per object its border pixels, how many of them have a foreign label
 *        within a distance, and its neighbours within that distance with their smallest squared distance, as exact
 *        integers in CSR rows (CellProfiler's MeasureObjectNeighbors; no reference counterpart)
 *   cs_label_colocalize
 *        how the channels go together inside the same objects: per object and pair of channels the sums behind Pearson's
 *        correlation, the regression slope, Manders' coefficients, the overlap and K coefficients and the rank-weighted
 *        coefficients, as exact integers (CellProfiler's MeasureColocalization; no reference counterpart)
 *   cs_label_radial
 *        where the intensity of the same objects sits between centre and outline: the exact depth of every object pixel
 *        (a per-label Euclidean distance transform), per object, ring and wedge the pixel count and the sums, and the
 *        records of the outline's intensities, as exact integers (CellProfiler's MeasureObjectIntensityDistribution and
 *        the Edge measures of MeasureObjectIntensity; no reference counterpart)
 *   cs_label_granularity
 *        the size spectrum of the bright structures inside the same objects: per spectrum step a grey-level erosion and
 *        a reconstruction by dilation of the whole plane, and per object, step and channel the sum of the reconstructed
 *        plane, as exact integers (CellProfiler's MeasureGranularity; no reference counterpart)
 *   cs_label_propagate
 *        grows the seeds of a label image inside a mask along the cheapest paths of an integer cost, geometric plus the
 *        differences of a guide stain: whole cells from nuclei (CellProfiler's IdentifySecondaryObjects "Propagation",
 *        skimage.segmentation.watershed with markers and a mask; no reference counterpart)
 *   cs_fit_scaler / cs_fit_pca_moments / cs_fit_pca_subspace / cs_fit_project / cs_fit_ocsvm
 *        RobustScaler / PCA / OneClassSVM fits of create_anomaly_detector
 *                                                 CAE_improved_modeltrain.py:408-427
 *   cs_synth_crops
 *        synthetic U[0,1) crops (no reference counterpart; benchmark/test input)
 *   cs_train_create / cs_train_step / cs_train_eval / cs_train_export
 *        the per-batch work of autoencoder.fit       CAE_improved_modeltrain.py:286-293
 *        on the model compiled at :223-227 (Adam 1e-3, loss 'mse', metric 'mae'); the
 *        callbacks of :263-283 are host-side scalars (cellscreen/training.py)
 *
 * Conventions
 *   - Every function returns CS_OK (0) or a negative cs_status.  cs_last_error()
 *     returns a thread-local message for the most recent failure on this thread.
 *   - Handles are opaque, created and destroyed by the library.  One handle = one
 *     device + one HIP stream + one workspace; a handle is not thread-safe, distinct
 *     handles are independent.  No exceptions or C++ types cross the boundary.
 *   - Every buffer passed in is caller-owned and borrowed for the duration of the call.
 *     `*_kind` says where it lives: CS_MEM_HOST (pageable or pinned host memory) or
 *     CS_MEM_DEVICE (memory of the handle's device, e.g. a torch tensor's data_ptr()).
 *   - Calls are synchronous: outputs are complete when the call returns.
 *   - Device INPUTS must be complete before the call: a handle works on its own non-blocking HIP
 *     stream, which is not ordered with any stream of the caller.  If a CS_MEM_DEVICE buffer (or a
 *     gradient buffer given to cs_train_set_grad_buffer) was produced by work still in flight on
 *     another stream -- a torch kernel, an RCCL collective -- either synchronise that stream, or
 *     call cs_model_wait_stream / cs_train_wait_stream / cs_fit_wait_stream /
 *     cs_preproc_wait_stream with it first (the Python wrappers do, with torch's current stream):
 *     the handle's next work then starts after everything enqueued on that stream so far.
 *   - Layouts: crops [n][H][W] fp32 (the trailing channel of 1 is implicit, as
 *     np.expand_dims at improved_detection.py:122 adds it); conv kernels HWIO
 *     [3][3][cin][cout] as Keras stores them; features [n][h*w*c] in (h,w,c) order
 *     as the reshape at improved_detection.py:131 produces.
 *   - The library links no communication library.  Multi-GPU is one process and one handle per GPU; every
 *     exchange between processes (the gradient all-reduce, the all-gather of BatchNormalization partials,
 *     the gather of results) happens ABOVE this ABI, in the host's own communicator (RCCL through
 *     torch.distributed in cellscreen/dist.py), on buffers the caller owns: cs_train_set_grad_buffer (the gradient) and
 *     cs_train_set_sync_bn / cs_train_set_sync_bn_stream (the BatchNormalization partials: a blocking hook, or one the
 *     caller orders on the handle's stream so that the host never waits) are the hooks.  Screening has no exchange on
 *     its data path.
 *   - There is NO CPU fallback: without a gfx950 device every compute entry point
 *     returns CS_ERR_NO_DEVICE.
 */
#ifndef CELLSCREEN_H
#define CELLSCREEN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CS_ABI_VERSION 2       /* 2: cs_model_options (precision) on cs_model_load / cs_model_from_arrays */
#define CS_MAX_CONV 16

typedef enum cs_status {
    CS_OK = 0,
    CS_ERR_INVALID = -1,      /* bad argument (NULL, negative size, wrong shape) */
    CS_ERR_IO = -2,           /* file missing / unreadable */
    CS_ERR_FORMAT = -3,       /* malformed model file */
    CS_ERR_NO_DEVICE = -4,    /* no usable gfx950 device */
    CS_ERR_HIP = -5,          /* HIP runtime error (message in cs_last_error) */
    CS_ERR_UNSUPPORTED = -6,  /* architecture / size this build has no kernel for */
    CS_ERR_NOMEM = -7,
    CS_ERR_NO_DETECTOR = -8   /* model was created without detector parameters */
} cs_status;

typedef enum cs_mem_kind { CS_MEM_HOST = 0, CS_MEM_DEVICE = 1 } cs_mem_kind;

typedef struct cs_model cs_model;

/* One conv autoencoder weight set (CAE_improved_modeltrain.py:184-229).
 * n_conv convs; the first n_enc are each followed by BatchNormalization + MaxPooling2D,
 * the next n_conv-n_enc-1 by BatchNormalization + UpSampling2D, the last has sigmoid.
 * BN arrays are NULL for the last conv. */
typedef struct cs_cae_weights {
    int32_t height, width;            /* input crop size: 64, 64 */
    int32_t n_conv, n_enc;            /* 7, 3 */
    int32_t channels[CS_MAX_CONV];    /* filters of each conv: 32,64,32,32,64,32,1 */
    const float *kernel[CS_MAX_CONV]; /* HWIO [3][3][cin][cout] */
    const float *bias[CS_MAX_CONV];   /* [cout] */
    const float *bn_gamma[CS_MAX_CONV];
    const float *bn_beta[CS_MAX_CONV];
    const float *bn_mean[CS_MAX_CONV];
    const float *bn_var[CS_MAX_CONV];
    float bn_eps;                     /* Keras default 1e-3 */
} cs_cae_weights;

/* One fitted OneClassSVM(kernel='rbf') (CAE_improved_modeltrain.py:420-427). */
typedef struct cs_ocsvm_params {
    int32_t n_sv;
    const double *support_vectors;    /* [n_sv][n_components]  (sklearn support_vectors_) */
    const double *dual_coef;          /* [n_sv]                (dual_coef_[0]) */
    double gamma;                     /* _gamma */
    double rho;                       /* -intercept_[0] == offset_[0] */
} cs_ocsvm_params;

/* RobustScaler + PCA + the two detectors (CAE_improved_modeltrain.py:408-427). */
typedef struct cs_detector_params {
    int32_t n_features;               /* 2048 */
    int32_t n_components;             /* <= 100 */
    const float *scaler_center;       /* [n_features]  center_  (float32) */
    const double *scaler_scale;       /* [n_features]  scale_   (float64) */
    const float *pca_components;      /* [n_components][n_features]  components_ */
    const float *pca_mean_proj;       /* [n_components] = mean_ @ components_.T (float32) */
    cs_ocsvm_params conservative;     /* nu = 0.05 */
    cs_ocsvm_params moderate;         /* nu = 0.10 */
} cs_detector_params;

/* How the fp32 contractions of the convs and of the PCA projection are evaluated.  Either way every tensor, bias,
 * BatchNormalization constant, accumulator and result is fp32 (the SVMs fp64), as in the reference
 * (improved_detection.py:122,125,130: Keras's float32 predict).
 *   CS_PRECISION_SPLIT16     (default) each fp32 operand as a two-term fp16 split (22 of 24 mantissa bits; exact
 *                            power-of-two scales per cell / strip) contracted by three products on the 16-bit
 *                            matrix instructions with fp32 accumulation; the PCA GEMM as a three-term bf16 split
 *                            (24 bits).  Inside every fp32 tolerance of tests/helpers.py; DESIGN.md section 3h.
 *   CS_PRECISION_FP32_EXACT  every contraction on v_mfma_f32_16x16x4_f32: fp32 operands, fp32 products, fp32
 *                            accumulation -- the reference's own arithmetic up to summation order.  ~0.58x the rate. */
typedef enum cs_precision { CS_PRECISION_SPLIT16 = 0, CS_PRECISION_FP32_EXACT = 1 } cs_precision;

/* Debug-only switches (A/B runs and the bit-identity tests): each keeps an UNFUSED form of the same arithmetic. */
#define CS_DEBUG_NO_FUSE12      0x1u   /* conv1 and conv2 as two kernels, p1 through HBM (conv2 as F(2x2,3x3): other bits) */
#define CS_DEBUG_NO_FUSE45      0x2u   /* conv4 and conv5 as two kernels, a4 through HBM (bit-identical) */
#define CS_DEBUG_NO_FUSE67      0x4u   /* conv6, conv7 + error as two kernels, a6 through HBM */
#define CS_DEBUG_NO_SMALL_SPLIT 0x8u   /* small calls keep the one-workgroup detector tail (bit-identical) */

/* Options of cs_model_load / cs_model_from_arrays; NULL = all defaults.  Set struct_size = sizeof(cs_model_options)
 * and zero the rest before filling in what is wanted. */
typedef struct cs_model_options {
    uint32_t struct_size;
    int32_t precision;                /* cs_precision */
    uint32_t debug_flags;             /* CS_DEBUG_* ; 0 in production */
    uint32_t reserved[5];             /* must be 0 */
} cs_model_options;

typedef struct cs_model_info {
    int32_t height, width;
    int32_t n_conv, n_enc;
    int32_t feature_dim;              /* h*w*c of the encoded tensor */
    int32_t n_components;
    int32_t n_sv_conservative, n_sv_moderate;
    int32_t shared_encoder;           /* 1: encoder weights are bit-identical to the
                                         autoencoder's encoder half, so one pass serves both */
    int32_t has_detector;
    int32_t device_id;
    int64_t chunk_cells;              /* cells processed per internal pass */
    int32_t channels[CS_MAX_CONV];    /* filters of each conv */
    int32_t reference_arch;           /* 1: the reference graph (tuned kernels); 0: generic-shape kernels */
    int32_t precision;                /* cs_precision the handle was created with */
    uint32_t debug_flags;
} cs_model_info;

/* ---- library / device ---------------------------------------------------------- */
int cs_abi_version(void);
const char *cs_status_string(int status);
const char *cs_last_error(void);
/* Number of visible HIP devices (0 if none).  Never fails. */
int cs_device_count(void);

/* ---- model --------------------------------------------------------------------- */
/* Reads <model_dir>/cae.bin (+ detector.bin if present) in the native tensor-archive
 * format written by cellscreen.model_io (see DESIGN.md "model_dir").
 * Replaces load_trained_models, improved_detection.py:23-46. */
int cs_model_load(const char *model_dir, int device_id, const cs_model_options *options, cs_model **out);

/* autoencoder: weights of best_autoencoder.keras (improved_detection.py:28).
 * encoder:     weights of encoder.keras (:29), n_conv = n_enc convs; NULL = same as the
 *              autoencoder's encoder half.  The two files may differ
 *              (CAE_improved_modeltrain.py:270-275 vs :300).
 * detector:    may be NULL; then cs_screen returns CS_ERR_NO_DETECTOR.
 * Architectures: the reference graph (64x64, filters 32-64-32 | 32-64-32-1) runs on kernels tuned for
 * it.  Any other instance of the same layer grammar -- create_improved_autoencoder(input_shape) is
 * generic in its input size (CAE_improved_modeltrain.py:184), e.g. BASELINE.json configs[4]: 128x128,
 * filters 32-64-128 | 128-64-32-1 -- runs on run-time-shaped MFMA kernels (csrc/conv_generic.hip):
 * n_conv = 2 n_enc + 1, last conv 1 filter, every conv grid's width a multiple of 16 and <= 128,
 * channel counts multiples of 4.  Anything else: CS_ERR_UNSUPPORTED.  Training handles (cs_train_*) take
 * the same architectures (cs_train_create). */
int cs_model_from_arrays(const cs_cae_weights *autoencoder, const cs_cae_weights *encoder,
                         const cs_detector_params *detector, int device_id, const cs_model_options *options,
                         cs_model **out);
void cs_model_free(cs_model *m);
/* Orders the handle's stream after all work enqueued so far on `hip_stream` (a hipStream_t; NULL = the legacy
 * default stream).  See "Device INPUTS" above.  Same for the three other handle types. */
int cs_model_wait_stream(cs_model *m, void *hip_stream);
int cs_model_get_info(const cs_model *m, cs_model_info *info);
/* Cells per internal pass (workspace ~0.4 MB per cell for the reference graph).  Default: automatic -- 16,384 for
 * host input (pipelined staging), up to 65,536 for device-resident input (a ~19 GB workspace for the reference graph);
 * this call fixes it, 0 returns to automatic.  The workspace is sized for min(n, chunk) cells of the largest call so far. */
int cs_model_set_chunk(cs_model *m, int64_t chunk_cells);

/* ---- the hot path -------------------------------------------------------------- */
/* compute_anomaly_scores, improved_detection.py:117-153, for n crops.
 * Outputs (each may be NULL to skip), all length n:
 *   mse, mae            reconstruction_mse / reconstruction_mae (float32)
 *   cons_score, mod_score   -decision_function (float64; "higher = more anomalous", :149-150)
 *   cons_pred, mod_pred     predict: +1 inlier / -1 anomaly (:138-139; libsvm dec > 0 ? 1 : -1)
 * n == 0 is valid and touches nothing (the reference returns {} at :119-120). */
int cs_screen(cs_model *m, const float *crops, int64_t n, int crops_kind,
              float *mse, float *mae, double *cons_score, double *mod_score,
              int8_t *cons_pred, int8_t *mod_pred, int out_kind);

/* autoencoder.predict + MSE/MAE (CAE_improved_modeltrain.py:335-339).
 * recon [n][H][W] may be NULL. */
int cs_reconstruct(cs_model *m, const float *crops, int64_t n, int crops_kind,
                   float *recon, float *mse, float *mae, int out_kind);

/* encoder.predict + reshape (improved_detection.py:130-131).
 * which = 0: the autoencoder's encoder half; 1: the encoder.keras weight set. */
int cs_encode(cs_model *m, const float *crops, int64_t n, int crops_kind, int which,
              float *features, int out_kind);

/* ---- stage taps for parity tests ------------------------------------------------ */
/* Output of conv `layer` (0-based) of the autoencoder after its relu/BN/pool (the tensor
 * the next conv reads), NHWC; for the last conv the sigmoid output.  out: n * layer size. */
int cs_layer_output(cs_model *m, const float *crops, int64_t n, int crops_kind, int layer,
                    float *out, int out_kind);
/* scaler.transform + pca.transform on caller-supplied features [n][n_features]. */
int cs_scaler_pca(cs_model *m, const float *features, int64_t n, int in_kind,
                  float *pca_out /* [n][n_components] */, int out_kind);
/* decision_function of both detectors on caller-supplied PCA vectors [n][n_components]. */
int cs_svm_decision(cs_model *m, const float *pca, int64_t n, int in_kind,
                    double *cons_dec, double *mod_dec, int out_kind);

/* ---- synthetic input ------------------------------------------------------------ */
/* Fills out_device[n][npix] with U[0,1) fp32 from the counter-based generator keyed
 * (seed, first_cell + i, pixel); bit-identical to oracle/cae_oracle.c:orc_synth_crops. */
int cs_synth_crops(cs_model *m, uint64_t seed, int64_t first_cell, int64_t n, int32_t npix,
                   float *out_device);

/* ---- crop preprocess (the caller side of the hot path) ----------------------------- */
/* What the reference does to every bounding-box crop before compute_anomaly_scores sees it
 * (improved_detection.py:98-99, CAE_improved_modeltrain.py:92-93):
 *     exposure.equalize_adapthist(crop, clip_limit=0.02)  ->  resize(., (out_h, out_w), anti_aliasing=True)
 * and the float32 cast of improved_detection.py:122.  Arithmetic of scikit-image 0.18.3 /
 * SciPy 1.7.1 (CLAHE bit-exact, resize in fp64).  Independent of cs_model: own handle, own stream.
 * The output size is state of the handle: 64 x 64 (the reference's resize) until
 * cs_preproc_set_output_size says otherwise -- the size a model of another input_shape reads.
 * Accepted, and refused outside (never clamped):
 *   output   8 <= out_h, out_w <= 512, independent of each other              (else CS_ERR_INVALID)
 *   crops    8 <= side <= 1024 per axis (below 8: CS_ERR_INVALID, skimage raises), and
 *            side <= 16 * out on that axis: the ratio bounds the anti-aliasing Gaussian's radius
 *            (sigma = (side/out - 1)/2 <= 7.5); at 64 it is the 1024 rule    (else CS_ERR_UNSUPPORTED)
 * A crop side below the output side is up-scaled: no filter along that axis, each axis by itself. */
typedef struct cs_preproc cs_preproc;
typedef enum cs_pixel_type { CS_PIX_U8 = 0, CS_PIX_U16 = 1 } cs_pixel_type;   /* TIFF channel dtypes */

int cs_preproc_create(int device_id, cs_preproc **out);
void cs_preproc_free(cs_preproc *p);
int cs_preproc_wait_stream(cs_preproc *p, void *hip_stream);
/* The output size of the handle (default 64 x 64); takes effect from the next cs_preprocess /
 * cs_extract_measure.  Sides outside [8, 512]: CS_ERR_INVALID, the size stays.  Between a successful
 * cs_extract_measure and its cs_extract_fill: CS_ERR_INVALID (the fill's buffers were sized by the measure). */
int cs_preproc_set_output_size(cs_preproc *p, int32_t out_h, int32_t out_w);
int cs_preproc_get_output_size(const cs_preproc *p, int32_t *out_h, int32_t *out_w);
/* pixels:  ragged buffer of n_pixels elements (pixels_kind: host or device); crop i is the
 *          row-major heights[i] x widths[i] block at element offsets[i].  offsets must ascend
 *          and crops must not overlap.  offsets/heights/widths are host arrays of length n.
 * Sides below 8 return CS_ERR_INVALID (kernel_size = shape // 8 would be 0: skimage raises),
 * above 1024 or above 16 x the output size on their axis CS_ERR_UNSUPPORTED (the message names the crop,
 * its sides and the output size); nothing is written then.
 * out:       [n][out_h][out_w] float32 (out_kind: host or device), the handle's output size.
 * clahe_out: optional stage tap, same layout/offsets as pixels (uint16, out_kind): the image
 *            skimage's _clahe returns before the final rescale.  Elements between crops: 0 / untouched.
 * n == 0 is valid and touches nothing. */
int cs_preprocess(cs_preproc *p, const void *pixels, int pixel_type, int64_t n_pixels, int pixels_kind,
                  const int64_t *offsets, const int32_t *heights, const int32_t *widths, int64_t n,
                  double clip_limit, float *out, uint16_t *clahe_out, int out_kind);
/* Device time (HIP events on the handle's stream around the kernel launches) and the pixel count
 * of the last cs_preprocess call. */
int cs_preproc_last_timing(const cs_preproc *p, double *kernel_ms, int64_t *pixels);

/* ---- quality-cell extraction from label images (improved_detection.py:61-111) ---------------
 * Input: B images of one shape H x W -- the analysis channel (uint8 / uint16) read in place from a
 * [B][H][W][channels] stack at `channel`, and int32 labels [B][H][W] from any segmenter (0 =
 * background).  Every label value > 0 present in an image is one region, connected or not, in
 * ascending label order per image (regionprops' order).  Per region, as the reference applies them:
 *   border        minr < border or minc < border or maxr > H-border or maxc > W-border (max exclusive)
 *   area          pixel count < min_area or > max_area
 *   eccentricity  > max_eccentricity; scikit-image 0.18.3's definition (inertia tensor of the central
 *                 moments, eigenvalues clipped at 0, sqrt(1 - l2/l1), 0 when l1 == 0) from exact int64
 *                 moment sums
 *   intensity     mean < min_mean or std < min_std, over the whole bbox rectangle of the analysis
 *                 channel (not masked: green_channel[minr:maxr, minc:maxc]), population std
 * and solidity = area / convex_area (reported, not filtered on): convex_area counts the bbox pixel
 * centres inside or on the convex hull of the region's pixel-edge midpoints (convex_hull_image with
 * offset_coordinates=True + grid_points_in_poly), exactly, in integer arithmetic.  Each passing
 * region's bbox crop goes through the cs_preprocess kernel on the device; the cells are bit-identical
 * to cs_preprocess on the same crops cut on the host.
 * Whole-image rules (status per image): a passing region with a bbox side < 8 makes skimage raise inside
 * the reference's per-file try (improved_detection.py:113-115), so the image yields no cells
 * (CS_IMAGE_NO_CELLS); a passing side > 1024, or > 16 x the handle's output size on its axis, is beyond
 * cs_preprocess (CS_IMAGE_UNSUPPORTED, no cells) -- the same rule, applied on the device.
 * The cells have the handle's output size (cs_preproc_set_output_size) as it was at cs_extract_measure.
 * Two calls per batch: cs_extract_measure runs the label pass, the per-region pass and the compaction
 * scan and returns the counts (one host synchronisation); cs_extract_fill writes the region table and
 * the cells (one more).  Between the two, CS_MEM_DEVICE inputs must stay valid and unchanged (the fill
 * reads the analysis channel again). */
typedef struct cs_qc_params {
    int32_t border;                   /* 10 */
    int32_t min_area, max_area;       /* 200, 8000 */
    int32_t reserved;                 /* must be 0 */
    double max_eccentricity;          /* 0.95 */
    double min_mean, min_std;         /* 0.5, 0.1 */
    double clip_limit;                /* 0.02: equalize_adapthist of the cells */
} cs_qc_params;

#define CS_QC_BORDER       0x1u       /* failed-rule bits of cs_region.failed */
#define CS_QC_AREA         0x2u
#define CS_QC_ECCENTRICITY 0x4u
#define CS_QC_INTENSITY    0x8u

#define CS_IMAGE_OK          0        /* per-image status of cs_extract_fill */
#define CS_IMAGE_NO_CELLS    1        /* a passing region has a bbox side < 8: the reference's extraction raises */
#define CS_IMAGE_UNSUPPORTED 2        /* a passing region has a bbox side > 1024 or > 16 x the output size */

/* One record per region, passing or not, in (image, label) order. */
typedef struct cs_region {
    int32_t image, label;
    int32_t minr, minc, maxr, maxc;   /* regionprops bbox, max exclusive */
    int64_t area, convex_area;
    double eccentricity, solidity;
    double mean_intensity, std_intensity;
    uint32_t failed;                  /* CS_QC_* bits of every rule the region fails; 0 = passes */
    int32_t cell;                     /* index of its cell in the output, -1 if none */
} cs_region;

/* image:  [batch][height][width][channels] uint8 / uint16 (pixel_type); the analysis channel is `channel`.
 * labels: [batch][height][width] int32.  Both in_kind.  Negative labels, or labels above max_label:
 *         CS_ERR_INVALID (detected on the device, reported by this call).
 * max_label: an upper bound of the batch's labels; it sizes the per-label tables.  Above 2^20, or
 *         batch * max_label above 2^22: CS_ERR_UNSUPPORTED (relabel sparse ids first: the order of the
 *         labels, and so every result, is kept by an order-preserving relabel).
 * height, width: 1..4096.  qc: NULL = the reference's values.
 * n_regions, n_cells: out, the sizes cs_extract_fill writes.  Without a gfx950 device (p == NULL because
 * cs_preproc_create failed): CS_ERR_NO_DEVICE. */
int cs_extract_measure(cs_preproc *p, const void *image, int pixel_type, int32_t channels, int32_t channel,
                       const int32_t *labels, int32_t batch, int32_t height, int32_t width, int in_kind,
                       int32_t max_label, const cs_qc_params *qc, int64_t *n_regions, int64_t *n_cells);
/* After cs_extract_measure on the same handle.  Each output may be NULL.
 *   regions      [n_regions] cs_region                         (table_kind)
 *   image_status [batch] int32 CS_IMAGE_*                      (table_kind)
 *   cells        [n_cells][out_h][out_w] float32, in region order (cells_kind)
 *   cell_image   [n_cells] int32: the image index of each cell (cells_kind) */
int cs_extract_fill(cs_preproc *p, cs_region *regions, int32_t *image_status, int table_kind, float *cells, int32_t *cell_image,
                    int cells_kind);
/* Device time of the last measure + fill: label pass, per-region pass (with the scan), gather + preprocess. */
int cs_extract_last_timing(const cs_preproc *p, double *label_ms, double *region_ms, double *cells_ms);

/* ---- built-in segmenter: global threshold + connected components ---------------------------
 * Not StarDist: a classical segmenter of the library's own, for bright cells on a dark background.
 * Touching cells come out as ONE region (the extraction's area / eccentricity rules then judge it) unless
 * cs_segment_split is called in its place, which cuts them apart at their necks, or cs_segment_split_intensity, which cuts
 * them along the intensity valleys between their cores.
 * Input as for the extraction: one `channel` of a [B][H][W][channels] uint8 / uint16 stack, read in place.
 *   threshold   CS_THRESH_OTSU: scikit-image 0.18.3's threshold_otsu of that channel of each image (exact
 *               integer histogram over [min, max], int64 cumulative sums, its float64 operations in its order:
 *               the same integer); a constant image gives its value.  CS_THRESH_FIXED: `threshold`.
 *               Foreground is pixel > threshold.
 *   fill_holes  background components (4-connected) that do not touch the image border become foreground:
 *               scipy.ndimage.binary_fill_holes with its default structure.
 *   labels      connected components of the mask, connectivity 1 (4 neighbours) or 2 (8), numbered 1.. in
 *               raster order of each component's first pixel: scipy.ndimage.label's and skimage.measure.label's
 *               numbering.  0 = background.
 * Integer arithmetic and integer atomics only: every output is bit-identical run to run and independent of
 * the other images of the batch. */
#define CS_THRESH_OTSU  0
#define CS_THRESH_FIXED 1
typedef struct cs_segment_params {
    int32_t threshold_mode;           /* CS_THRESH_OTSU / CS_THRESH_FIXED */
    int32_t threshold;                /* FIXED: 0..65535; ignored by OTSU */
    int32_t connectivity;             /* 1 or 2 */
    int32_t fill_holes;               /* 0 or 1 */
} cs_segment_params;                  /* NULL = OTSU, connectivity 1, no hole filling */

/* image:  [batch][height][width][channels] uint8 / uint16 (pixel_type), in_kind.  height, width: 1..4096
 *         (above: CS_ERR_UNSUPPORTED, as the extraction: a deliberate difference from the CS_ERR_INVALID of the other bad
 *         arguments); batch: 1..65535 (the launch grid's bound).  Workspace on the device: 5 bytes per pixel (mask and
 *         parents; 4 more for labels that go to the host), and for CS_THRESH_OTSU the histogram tables: 2 KB per image for
 *         uint8, 256 KB x (1 + parts) per image for uint16 with parts = min(16, 256 / batch, pixels / 16384) >= 1 -- 2.3 MB
 *         per image at batch 32, 0.5 MB from batch 256 on.  A batch whose workspace does not fit returns CS_ERR_NOMEM;
 *         split it (the results do not depend on the batch).
 * labels: out, [batch][height][width] int32, labels_kind.  Left on the device they are cs_extract_measure's
 *         `labels` as they are, on the same handle, with max_label = the largest of n_labels (counts beyond the
 *         extraction's table limits are the extraction's to refuse).
 * n_labels:   out, host [batch]: components per image.
 * thresholds: out, host [batch], or NULL: the threshold used per image.
 * One host synchronisation per call.  Bad arguments: CS_ERR_INVALID before any device work; without a gfx950
 * device (p == NULL because cs_preproc_create failed): CS_ERR_NO_DEVICE. */
int cs_segment_threshold(cs_preproc *p, const void *image, int pixel_type, int32_t channels, int32_t channel,
                         int32_t batch, int32_t height, int32_t width, int in_kind,
                         const cs_segment_params *params, int32_t *labels, int labels_kind,
                         int32_t *n_labels, int32_t *thresholds);
/* Device time of the last cs_segment_threshold: histogram + threshold + mask, and hole filling + labelling. */
int cs_segment_last_timing(const cs_preproc *p, double *threshold_ms, double *label_ms);

/* cs_segment_threshold with touching cells split: a distance-transform watershed on the same mask (after the threshold and
 * the optional hole filling), exact and all integers.  The result is a function of the mask alone:
 *   Dq     min(isqrt(4 * D2), 255): D2 the exact squared Euclidean distance of a foreground pixel to the nearest
 *          background pixel of the same image (scipy.ndimage.distance_transform_edt squared), so Dq is the distance in half
 *          pixels; 0 on background.  Outside the image is not background; an image without background is 255 everywhere.
 *   seeds  R = morphological reconstruction by dilation of max(Dq - h, 0) under Dq; the seeds are the regional maxima of R
 *          inside the mask (the h-maxima of Dq), numbered in raster order of their first pixels.
 *   flood  for v = 255 .. 1: an unlabelled pixel with Dq >= v takes the label that reaches it through unlabelled pixels
 *          with Dq >= v with the smallest (number of steps, label); the step count restarts at every level.
 *   labels the regions, renumbered 1.. in raster order of each region's first pixel.  Where every component holds one
 *          seed they equal cs_segment_threshold's labels bit for bit.
 * The segmenter's connectivity is the neighbourhood of the dilation, the plateaus and the steps.  With connectivity 2 the
 * chessboard step count skews the cut between two equal cells; connectivity 1 is the default.  Not split: cells that
 * overlap without a neck (one maximum), and cores deeper than 127 px (one plateau of Dq = 255).
 * Workspace on the device beyond cs_segment_threshold's: 10 bytes per pixel and 1 byte per 64 x 16 tile.  Host
 * synchronisations: one per 16 rounds of the reconstruction, one per 64 rounds of the flood and the final one -- 3 for
 * isolated small cells, a handful for crowded fields.  Arguments, errors and outputs as cs_segment_threshold; h outside 1..255:
 * CS_ERR_INVALID.
 * dist: optional out, [batch][height][width] uint8: Dq, on the device or the host as labels_kind; NULL: not wanted. */
typedef struct cs_split_params {
    int32_t h;                        /* half pixels, 1..255: how much lower than its peak a saddle must be to separate two cells */
} cs_split_params;                    /* NULL = h 3 */
int cs_segment_split(cs_preproc *p, const void *image, int pixel_type, int32_t channels, int32_t channel,
                     int32_t batch, int32_t height, int32_t width, int in_kind,
                     const cs_segment_params *params, const cs_split_params *split, int32_t *labels, int labels_kind,
                     int32_t *n_labels, int32_t *thresholds, uint8_t *dist);
/* Device time of the last cs_segment_split: histogram + threshold + mask; hole filling + distances; reconstruction + seeds;
 * flood + numbering. */
int cs_segment_split_last_timing(const cs_preproc *p, double *threshold_ms, double *distance_ms, double *seed_ms,
                                 double *flood_ms);

/* cs_segment_split with the heights taken from the image instead of from the mask: cells that overlap without a neck, which the
 * distance split leaves whole, are cut along the darker valley between their bright cores.  Exact and all integers; the result is
 * a function of the mask (after the threshold and the optional hole filling) and of the guide plane G alone:
 *   lo_c, hi_c   the smallest and largest G over the pixels of component c of the mask (under the connectivity; filled holes
 *                count);
 *   Hq     1 + ((G - lo_c) * 254) / max(hi_c - lo_c, min_contrast, 1) on the mask, a byte in 1..255; 0 on background.  The scale
 *          is per component: a dim cell beside a bright field keeps its own 254 levels, and the result does not depend on the
 *          rest of the batch.  A component flatter than min_contrast is not stretched to the full range (the guard against
 *          splitting on noise); a constant component is 1 everywhere.
 *   R, seeds, flood, labels   as cs_segment_split, with Hq in Dq's place and depth in h's: two cores are separated when the
 *          valley between them lies at least `depth` of the component's 254 levels below the lower core.
 * With depth 254 every component holds one seed and the labels equal cs_segment_threshold's bit for bit; adding a constant to G
 * changes nothing.  G must be smooth (cs_segment_smooth's plane): on a noisy plane every noise peak deeper than `depth` is a
 * seed.  Cells that overlap in projection add up, so the lens between two cores can be the brightest spot: a third region.
 * guide: the plane G, [batch][height][width][guide_channels] of guide_pixel_type, where `image` is (in_kind); channel
 *        guide_channel is read in place.  It may be `image` itself; with cs_segment_local or cs_segment_clean in front, `image`
 *        is their 0 / 1 plane and `guide` the plane they were made from.
 * height: optional out, [batch][height][width] uint8: Hq, on the device or the host as labels_kind; NULL: not wanted.
 * Workspace and host synchronisations as cs_segment_split (the component ranges live in the flood's key buffer), and a copy of
 * a guide that comes from the host.  NULL split or guide, depth outside 1..254, min_contrast outside 0..65535, non-zero reserved,
 * a bad guide pixel type or channel: CS_ERR_INVALID before any device work; everything else as cs_segment_split. */
typedef struct cs_split_intensity_params {
    int32_t depth;                    /* 1..254 levels: how much lower than its peak a valley must be to separate two cores */
    int32_t min_contrast;             /* 0..65535 counts: a component's range is stretched over at least this much */
    int32_t reserved[2];              /* 0 */
} cs_split_intensity_params;
int cs_segment_split_intensity(cs_preproc *p, const void *image, int pixel_type, int32_t channels, int32_t channel,
                               int32_t batch, int32_t height_px, int32_t width, int in_kind,
                               const cs_segment_params *params, const cs_split_intensity_params *split,
                               const void *guide, int guide_pixel_type, int32_t guide_channels, int32_t guide_channel,
                               int32_t *labels, int labels_kind, int32_t *n_labels, int32_t *thresholds, uint8_t *height);
/* Device time of the last cs_segment_split_intensity: histogram + threshold + mask; hole filling + components + heights;
 * reconstruction + seeds; flood + numbering. */
int cs_segment_split_intensity_last_timing(const cs_preproc *p, double *threshold_ms, double *height_ms, double *seed_ms,
                                           double *flood_ms);

/* Host synchronisations of the last cs_segment_split or cs_segment_split_intensity on this handle beyond the final one: the
 * reads of the control word after a group of 16 reconstruction rounds and after a group of 64 flood rounds. */
int cs_segment_split_last_syncs(const cs_preproc *p, int32_t *reconstruction, int32_t *flood);

/* Background correction of the segmentation channel before the threshold: for images whose illumination is not flat
 * (vignetting, a tilted coverslip, out-of-focus haze), where one global threshold cuts the field in two instead of finding
 * cells.  Integer arithmetic in the pixel type, each image on its own:
 *   median   (optional) the 3 x 3 median with the edge pixel repeated: scipy.ndimage.median_filter(x, size=3), default mode.
 *   top-hat  out = x - dilate(erode(x)) with the flat square of side 2 * radius + 1, erosion and dilation being the minimum
 *            and maximum over the window [i - r, i + r] x [j - r, j + r] clipped to the image:
 *            scipy.ndimage.white_tophat(x, size=(2r + 1, 2r + 1)) bit for bit, also where r exceeds a side.  The opening is
 *            never above x, so the subtraction cannot wrap.
 * radius must exceed half the width of the widest cell, or the opening eats the cell's core: the extraction's area limit of
 * 8000 px (a disk of diameter 101) asks for radius >= 51 where cells get that large.  The cost does not grow with the radius
 * beyond the halo a tile reads (at most the tile again).
 * image, pixel_type, channels, channel, batch, height, width, in_kind: as cs_segment_threshold; the channel is read in place.
 * out: [batch][height][width] of the same pixel type, out_kind.  Left on the device it is cs_segment_threshold's or
 *      cs_segment_split's `image` with channels = 1, channel = 0, on the same handle (the same stream: no ordering needed).
 * Workspace on the device: 2 planes of the pixel type (2 or 4 bytes per pixel), one more with the median, one more for an
 * `out` on the host, and the image itself when it comes from the host.
 * Host synchronisations: none when image and out are both on the device (the plane is complete in stream order; the times
 * are read when cs_segment_background_last_timing asks for them, which waits for the plane), else one.
 * Bad arguments (NULL params among them, radius outside 1..255, median not 0 or 1): CS_ERR_INVALID before any device work;
 * sides above 4096, batches above 65535: CS_ERR_UNSUPPORTED; without a gfx950 device (p == NULL): CS_ERR_NO_DEVICE. */
typedef struct cs_background_params {
    int32_t radius;                   /* 1..255: the square has side 2 * radius + 1 */
    int32_t median;                   /* 0 or 1: 3 x 3 median first */
} cs_background_params;
int cs_segment_background(cs_preproc *p, const void *image, int pixel_type, int32_t channels, int32_t channel,
                          int32_t batch, int32_t height, int32_t width, int in_kind,
                          const cs_background_params *params /* not NULL */, void *out, int out_kind);
/* Device time of the last cs_segment_background: the median (0 without it) and the four passes of the top-hat.  Waits for
 * that call's plane if it was left on the device. */
int cs_segment_background_last_timing(const cs_preproc *p, double *median_ms, double *tophat_ms);

/* Local mean threshold: a mask from each pixel's own neighbourhood instead of one global number, for fields that hold bright
 * and dim cells side by side (Otsu settles between the background and the bright population, and the dim cells fall under
 * it; the top-hat above removes an additive background, not a difference in brightness).  Integers only, each image on its own:
 *   median  (optional) the 3 x 3 median of cs_segment_background first; both sides of the comparison then see its plane.
 *   S(i,j)  the sum of x over the window [i - r, i + r] x [j - r, j + r] (side w = 2 * radius + 1, n = w * w pixels), indices
 *           outside the image reflected about the edge (d c b a | a b c d: scipy's mode='reflect', numpy.pad's 'symmetric',
 *           period 2 * side, so radius may exceed a side).
 *   out     1 where n * x - S - n * delta > 0 and x > floor, else 0 (64-bit arithmetic: n * x reaches 1.7e10).
 * This is x > skimage.filters.threshold_local(x, w, method='mean', offset=-delta), decided exactly.  The one deliberate
 * difference: where n * (x - delta) = S the pixel is background, while the library's float64 mean may fall on either side of
 * such a tie.  Everywhere else the two agree (the mean's rounding error is far below the smallest non-zero gap, 1 / n).
 * The window must be wider than the widest cell (as the top-hat's square), or a cell's core sits near its own mean and drops
 * out.  Noise on empty background passes a small delta as speckle: a delta of a few noise sigmas and median = 1 keep it down.
 * image, pixel_type, channels, channel, batch, height, width, in_kind: as cs_segment_threshold; the channel is read in place.
 *      The output of cs_segment_background is a valid image (channels = 1, channel = 0): the local rule after the top-hat.
 * out: [batch][height][width] uint8, out_kind.  Left on the device it is cs_segment_threshold's or cs_segment_split's `image`
 *      with pixel_type CS_PIX_U8, channels = 1, channel = 0, CS_THRESH_FIXED and threshold = 0, on the same handle (the same
 *      stream: no ordering needed); hole filling, labels and the split follow unchanged.
 * Workspace on the device: 4 bytes per pixel (the row sums), one plane of the pixel type more with the median (1 or 2 bytes
 * per pixel), 1 byte per pixel for an `out` on the host, and the image itself when it comes from the host.
 * Host synchronisations: none when image and out are both on the device (the plane is complete in stream order; the times
 * are read when cs_segment_local_last_timing asks for them, which waits for the plane), else one.
 * Bad arguments (NULL params among them, radius outside 1..255, delta outside -65535..65535, floor outside -1..65535, median
 * not 0 or 1): CS_ERR_INVALID before any device work; sides above 4096, batches above 65535: CS_ERR_UNSUPPORTED; without a
 * gfx950 device (p == NULL): CS_ERR_NO_DEVICE. */
typedef struct cs_local_params {
    int32_t radius;                   /* 1..255: the window has side 2 * radius + 1 */
    int32_t delta;                    /* -65535..65535: counts above the local mean */
    int32_t floor;                    /* -1..65535: pixel > floor as well; -1 = off */
    int32_t median;                   /* 0 or 1: 3 x 3 median first */
} cs_local_params;
int cs_segment_local(cs_preproc *p, const void *image, int pixel_type, int32_t channels, int32_t channel,
                     int32_t batch, int32_t height, int32_t width, int in_kind,
                     const cs_local_params *params /* not NULL */, uint8_t *out, int out_kind);
/* Device time of the last cs_segment_local: the median (0 without it), and the two sum passes with the comparison.  Waits for
 * that call's plane if it was left on the device. */
int cs_segment_local_last_timing(const cs_preproc *p, double *median_ms, double *sum_ms);

/* Mask cleanup between the hole filling and the labelling: speckle that passes the threshold (noise under a small local delta,
 * above all) and bridges of a few pixels between cells leave the mask before anything is labelled, flooded or measured.
 * Integers only, each image on its own, in this order:
 *   mask      cs_segment_threshold's: pixel > threshold (Otsu's or the fixed one) of the channel, hole-filled with fill_holes.
 *   opening   open_radius erosions, then as many dilations, by the 3 x 3 cross (open_connectivity 1: a diamond of that radius
 *             in all) or the 3 x 3 square (2: the square of side 2 * open_radius + 1); outside the image is background for the
 *             erosion: scipy.ndimage.binary_opening(mask, generate_binary_structure(2, open_connectivity),
 *             iterations=open_radius) bit for bit.  The square rounds a disk's diagonal edge by about 0.4 * open_radius px.
 *   min area  components of the opened mask under params->connectivity with fewer than min_area pixels become background:
 *             skimage.morphology.remove_small_objects(mask, min_size=min_area, connectivity=params->connectivity); a component
 *             of exactly min_area pixels stays.
 * image, pixel_type, channels, channel, batch, height, width, in_kind, params: as cs_segment_threshold.  The outputs of
 *      cs_segment_background and cs_segment_local are valid images (channels = 1, channel = 0; the latter with pixel_type
 *      CS_PIX_U8, CS_THRESH_FIXED and threshold = 0).
 * out: [batch][height][width] uint8, 0 / 1, out_kind.  Left on the device it is cs_segment_threshold's or cs_segment_split's
 *      `image` with pixel_type CS_PIX_U8, channels = 1, channel = 0, CS_THRESH_FIXED, threshold = 0 and fill_holes = 0, on the
 *      same handle (the same stream: no ordering needed).
 * thresholds: out, host [batch], or NULL: the threshold used per image.
 * Workspace on the device: cs_segment_threshold's with labels that go to the host (9 bytes per pixel, and the histogram tables
 * for CS_THRESH_OTSU), 1 byte per pixel more for an `out` on the host, and the image itself when it comes from the host.
 * Host synchronisations: none when image and out are both on the device and thresholds is NULL (the plane is complete in
 * stream order; the times are read when cs_segment_clean_last_timing asks for them, which waits for the plane), else one.
 * Bad arguments (NULL clean among them, open_radius outside 0..15, open_connectivity not 1 or 2, min_area outside 0..2^24, both
 * steps off): CS_ERR_INVALID before any device work; sides above 4096, batches above 65535: CS_ERR_UNSUPPORTED; without a
 * gfx950 device (p == NULL): CS_ERR_NO_DEVICE. */
typedef struct cs_clean_params {
    int32_t open_radius;              /* 0 = none, 1..15 */
    int32_t open_connectivity;        /* 1 cross, 2 square */
    int32_t min_area;                 /* 0 = none, 1..16777216 */
} cs_clean_params;
int cs_segment_clean(cs_preproc *p, const void *image, int pixel_type, int32_t channels, int32_t channel,
                     int32_t batch, int32_t height, int32_t width, int in_kind,
                     const cs_segment_params *params, const cs_clean_params *clean /* not NULL */,
                     uint8_t *out, int out_kind, int32_t *thresholds /* may be NULL */);
/* Device time of the last cs_segment_clean: threshold + mask + hole filling, the opening (0 without it), and the labelling,
 * counting and dropping of the area step (0 without it).  Waits for that call's plane if it was left on the device. */
int cs_segment_clean_last_timing(const cs_preproc *p, double *mask_ms, double *open_ms, double *area_ms);

/* Hysteresis threshold, in the place of the plain cut (or of cs_segment_local): two rules of one form instead of one.  A pixel is
 * foreground if it passes the weak rule and is connected, through pixels that pass it too, to a pixel that passes the strong
 * rule: skimage.filters.apply_hysteresis_threshold, decided in integers.  Speckle has no strong pixel and goes whatever its
 * size; a cell keeps its whole weak extent.  Each image on its own:
 *   strong    the rule there is without this stage.  Global: x > t_b, t_b Otsu's threshold of image b or the fixed one.
 *             CS_WEAK_LOCAL: n * x - S - n * local->delta > 0 and x > local->floor, as cs_segment_local.
 *   weak      CS_WEAK_ABSOLUTE: x > low_b, low_b = min(weak, t_b), weak in counts (0..65535; with CS_THRESH_FIXED not above the
 *             threshold).  CS_WEAK_FRACTION: low_b = (t_b * weak) >> 16, weak = q in 1..65535, a fraction q / 65536 of the strong
 *             threshold: the form for CS_THRESH_OTSU, where t_b is not known in advance.  CS_WEAK_LOCAL: the strong rule with the
 *             delta `weak` (-65535..65535, not above local->delta) in local->delta's place; window, reflected edges, floor and
 *             tie rule (an exact tie is background) are the same.  So every strong pixel is a weak pixel.
 *   result    the pixels of those components of the weak mask, under params->connectivity, that hold at least one strong pixel.
 *             With low_b = t_b (or weak = local->delta) it is the plain mask.
 * image, pixel_type, channels, channel, batch, height, width, in_kind, params: as cs_segment_threshold; with CS_WEAK_LOCAL
 *      params->threshold_mode and params->threshold are not read.  params->fill_holes is checked and NOT applied: the plane is
 *      taken before the hole filling, which the labelling call after it does (see out).
 * local: the local rule's parameters with CS_WEAK_LOCAL (its median runs once, here), NULL otherwise.
 * out: [batch][height][width] uint8, 0 / 1, out_kind.  Left on the device it is cs_segment_threshold's, cs_segment_split's or
 *      cs_segment_clean's `image` with pixel_type CS_PIX_U8, channels = 1, channel = 0, CS_THRESH_FIXED and threshold = 0, on
 *      the same handle (the same stream: no ordering needed); hole filling, cleanup, labels and the split follow unchanged.
 * thresholds: out, host [batch], or NULL: the strong rule's threshold per image; -1 with CS_WEAK_LOCAL (no single number).
 * Workspace on the device: cs_segment_threshold's with labels that go to the host (9 bytes per pixel, and the histogram tables
 * for CS_THRESH_OTSU; the 4 bytes of the labels hold one flag per root), with CS_WEAK_LOCAL cs_segment_local's sums and median
 * plane, 1 byte per pixel more for an `out` on the host, and the image itself when it comes from the host.
 * Host synchronisations: none when image and out are both on the device and no threshold has to be read (thresholds NULL, or
 * CS_WEAK_LOCAL); the plane is then complete in stream order and the times are read when cs_segment_hysteresis_last_timing asks
 * for them, which waits for the plane.  Else one.
 * Bad arguments (NULL hysteresis among them, an unknown mode, weak out of its mode's range or above the strong number, reserved
 * not 0, local missing with CS_WEAK_LOCAL or given without it): CS_ERR_INVALID before any device work; sides above 4096, batches
 * above 65535: CS_ERR_UNSUPPORTED; without a gfx950 device (p == NULL): CS_ERR_NO_DEVICE. */
enum { CS_WEAK_ABSOLUTE = 0, CS_WEAK_FRACTION = 1, CS_WEAK_LOCAL = 2 };
typedef struct cs_hysteresis_params {
    int32_t mode;                     /* CS_WEAK_ABSOLUTE, CS_WEAK_FRACTION or CS_WEAK_LOCAL */
    int32_t weak;                     /* counts, q (fraction q / 65536), or the weak delta */
    int32_t reserved[2];              /* 0 */
} cs_hysteresis_params;
int cs_segment_hysteresis(cs_preproc *p, const void *image, int pixel_type, int32_t channels, int32_t channel,
                          int32_t batch, int32_t height, int32_t width, int in_kind,
                          const cs_segment_params *params, const cs_local_params *local /* NULL unless CS_WEAK_LOCAL */,
                          const cs_hysteresis_params *hysteresis /* not NULL */,
                          uint8_t *out, int out_kind, int32_t *thresholds /* may be NULL */);
/* Device time of the last cs_segment_hysteresis: everything up to the level plane (thresholds or median and sums, and the
 * comparison), then the weak components, the flags and the kept plane.  Waits for that call's plane if it was left on the
 * device. */
int cs_segment_hysteresis_last_timing(const cs_preproc *p, double *level_ms, double *link_ms);

/* Noise-adaptive threshold, in the place of the plain cut, of cs_segment_local or of cs_segment_hysteresis: foreground is
 * "k sigmas above the local background", both estimated from the image itself on a coarse mesh of tiles, as SExtractor and
 * photutils' Background2D cut.  One dimensionless number serves every exposure, camera and bit depth, a sloping background needs
 * no top-hat, and a second k gives the hysteresis pair.  Integers only, no tolerance anywhere, each image on its own; x is the
 * channel:
 *   mesh      tile side T = tile.  Along an axis of n pixels there are m = max(1, n / T) tiles; tile i covers [i T, (i + 1) T),
 *             the last one runs to n (at most 2T - 1 wide).  An image smaller than T is one tile.
 *   tile      over the tile's N pixels: med = the value of rank (N - 1) / 2 in sorted order (the lower median), dev = the value
 *             of the same rank among |x - med|; B8 = 256 med, S8 = max((dev * 97164) >> 8, floor8): 97164 = 1.4826 * 65536, so
 *             S8 is the Gaussian-equivalent sigma in 1/256 counts; floor8 guards flat or clipped backgrounds, where dev = 0.
 *   filter    B8 and S8 are each replaced by the median (fifth of nine) of their 3 x 3 mesh neighbourhood, the mesh replicated
 *             at its edges: a tile that a cell fills is rejected.
 *   maps      bilinear between tile centres, constant outside the outer centres, without a division: along an axis node i sits
 *             at the doubled coordinate C2_i = start_i + end_i - 1 (end exclusive); for pixel p take i with C2_i <= 2p < C2_(i+1),
 *             clamped to the first or last pair of nodes; D = C2_(i+1) - C2_i, w1 = clamp(2p - C2_i, 0, D), w0 = D - w1; an axis
 *             with a single node has D = 1, w0 = 1.  N_B(y, x) = sum over the four nodes of wy * wx * B8, N_S the same sum of S8,
 *             D = Dy * Dx.
 *   rule      a pixel v is foreground iff 256 * (256 * v * D - N_B) > k8 * N_S (64-bit: D < 2^20, N_S < 2^45, k8 < 2^14); an
 *             exact tie is background, as in cs_segment_local.
 *   weak      weak_k8 != -1: the same inequality with weak_k8 (1..k8) is the weak rule, and the result keeps the components of
 *             the weak mask, under `connectivity`, that hold a strong pixel, as cs_segment_hysteresis does with its two rules.
 * image, pixel_type, channels, channel, batch, height, width, in_kind: as cs_segment_threshold; the channel is read in place.
 *      The outputs of cs_segment_smooth and cs_segment_background are valid images (channels = 1, channel = 0).
 * out: [batch][height][width] uint8, 0 / 1, out_kind.  Left on the device it is cs_segment_threshold's, cs_segment_split's or
 *      cs_segment_clean's `image` with pixel_type CS_PIX_U8, channels = 1, channel = 0, CS_THRESH_FIXED and threshold = 0, on
 *      the same handle (the same stream: no ordering needed); hole filling, cleanup, labels and the split follow unchanged.
 * mesh: out, host [batch][2][my][mx] int32, or NULL: the mesh after the filter, B8 then S8 (my, mx: the tiles along height, width).
 * Workspace on the device: the mesh, two int32 per tile before the filter and two after; with a weak rule cs_segment_threshold's
 * with labels that go to the host (9 bytes per pixel; the 4 bytes of the labels hold one flag per root); 1 byte per pixel more
 * for an `out` on the host, and the image itself when it comes from the host.
 * Host synchronisations: none when image and out are both on the device and mesh is NULL (the plane is complete in stream
 * order; the times are read when cs_segment_noise_last_timing asks for them, which waits for the plane), else one.
 * Bad arguments (NULL noise among them, tile not a power of two in 16..256, k8 outside 1..16383, weak_k8 neither -1 nor in
 * 1..k8, floor8 outside 0..4095 * 256, with a weak rule connectivity not 1 or 2, reserved not 0): CS_ERR_INVALID before any
 * device work; sides above 4096, batches above 65535: CS_ERR_UNSUPPORTED; without a gfx950 device (p == NULL):
 * CS_ERR_NO_DEVICE. */
typedef struct cs_noise_params {
    int32_t tile;                     /* 16, 32, 64, 128 or 256: the side of a mesh tile */
    int32_t k8;                       /* 1..16383: k in 1/256, int(k * 256 + 0.5) */
    int32_t weak_k8;                  /* -1: no weak rule, else 1..k8 */
    int32_t floor8;                   /* 0..4095 * 256: the least sigma in 1/256 counts */
    int32_t connectivity;             /* 1 or 2; read with a weak rule */
    int32_t reserved[3];              /* 0 */
} cs_noise_params;
int cs_segment_noise(cs_preproc *p, const void *image, int pixel_type, int32_t channels, int32_t channel,
                     int32_t batch, int32_t height, int32_t width, int in_kind,
                     const cs_noise_params *noise /* not NULL */, uint8_t *out, int out_kind,
                     int32_t *mesh /* may be NULL */);
/* Device time of the last cs_segment_noise: the tile statistics and the mesh filter, the cut (or the level plane), and with a
 * weak rule the weak components, the flags and the kept plane (0 without it).  Waits for that call's plane if it was left on
 * the device. */
int cs_segment_noise_last_timing(const cs_preproc *p, double *mesh_ms, double *cut_ms, double *link_ms);

/* Gaussian smoothing of the segmentation channel, before everything else: for noisy fields, where the threshold shatters a
 * faint cell into fragments that no cleanup of the mask can put together again.  Integers only, each image on its own:
 *   median  (optional) the 3 x 3 median of cs_segment_background first: hot pixels go before they are smeared.
 *   T(i,j)  sum over k = -radius..radius of weights[|k|] * x(i, fold(j + k, width))      (fits 32 bits)
 *   A(i,j)  sum over k of weights[|k|] * T(fold(i + k, height), j)                       (below 2^48)
 *   plane   (A + 2^31) >> 32: one rounding to nearest, at the very end.
 * fold reflects an index about the edges (d c b a | a b c d: scipy's mode='reflect', as cs_segment_local; period 2 * side, so
 * radius may exceed a side).  The table is part of the input: any non-negative weights with weights[0] >= 1 and weights[0] +
 * 2 * (weights[1] + ... + weights[radius]) == 65536 are applied exactly; a constant image maps to itself and nothing can
 * overflow.  cellscreen.segment.smooth_weights(sigma) builds the table of a Gaussian: radius = int(4 * sigma + 0.5), taps
 * proportional to exp(-k^2 / (2 sigma^2)), rounded down, the rest handed out by largest remainder.  With it the plane is
 * scipy.ndimage.gaussian_filter(x, sigma, mode='reflect', truncate=4.0) computed in float64, to within 0.5 + top * (2 eps + eps^2),
 * eps being the summed quantisation error of the taps; the library's own integer output truncates and is not
 * reproduced bit for bit.
 * image, pixel_type, channels, channel, batch, height, width, in_kind: as cs_segment_threshold; the channel is read in place.
 * plane: [batch][height][width] of the same pixel type, plane_kind.  Left on the device it is the `image` of every other
 *      cs_segment_* call with channels = 1, channel = 0, on the same handle (the same stream: no ordering needed).
 * Workspace on the device: 4 bytes per pixel (the row pass), one plane of the pixel type more with the median, one more for a
 * `plane` on the host, and the image itself when it comes from the host; CS_ERR_NOMEM when it does not fit.
 * Host synchronisations: none when image and plane are both on the device (the plane is complete in stream order; the times
 * are read when cs_segment_smooth_last_timing asks for them, which waits for the plane), else one.
 * Bad arguments (NULL params among them, radius outside 1..64, median not 0 or 1, reserved not 0, a negative weight,
 * weights[0] < 1, a non-zero weight beyond radius, a sum other than 65536): CS_ERR_INVALID before any device work; sides above
 * 4096, batches above 65535: CS_ERR_UNSUPPORTED; without a gfx950 device (p == NULL): CS_ERR_NO_DEVICE. */
typedef struct cs_smooth_params {
    int32_t radius;                   /* 1..64 */
    int32_t median;                   /* 0 or 1: 3 x 3 median first */
    int32_t weights[65];              /* weights[k]: the tap at distance k, k = 0..radius; beyond radius: 0 */
    int32_t reserved;                 /* must be 0 */
} cs_smooth_params;
int cs_segment_smooth(cs_preproc *p, const void *image, int pixel_type, int32_t channels, int32_t channel,
                      int32_t batch, int32_t height, int32_t width, int in_kind,
                      const cs_smooth_params *params /* not NULL */, void *plane, int plane_kind);
/* Device time of the last cs_segment_smooth: the median (0 without it) and the two passes.  Waits for that call's plane if it
 * was left on the device. */
int cs_segment_smooth_last_timing(const cs_preproc *p, double *median_ms, double *smooth_ms);

/* ---- scoring label images against ground truth ------------------------------------------------ */
/* Object matching by intersection over union between two label images per field, `pred` and `truth` (0 = background, every
 * value > 0 that occurs is one object, connected or not).  The device makes the tables below; TP / FP / FN, precision, recall,
 * F1 and panoptic quality at any IoU threshold in [0.5, 1] follow from them on the host in integers (cellscreen/score.py,
 * DESIGN 3s).  With A the pixel count of an object and I(p, t) that of an intersection, per image:
 *   area     A of the object
 *   partner  the object of the other image with the largest I; ties go to the smaller label; 0 when it meets none
 *   overlap  I with the partner
 *   n_major  the number of objects of the other image that lie mostly inside this one: 2 * I > A_other
 * A pair (p, t) matches at tq / 65536 when p and t are each other's partner, 2 * I > U and I * 65536 >= tq * U, where
 * U = A_p + A_t - I: the strict 2 * I > U makes the candidate of an object unique, so no assignment problem is solved.
 * pred, truth: [batch][height][width] int32, both in_kind.  Left on the device by cs_segment_* on this handle they are read in
 *         stream order, as cs_extract_measure reads them.  height, width 1..4096, batch 1..65535 (above: CS_ERR_UNSUPPORTED).
 * max_pred, max_truth: 1..2^20, batch * max at most 2^22 for each (above: CS_ERR_UNSUPPORTED).  A label that is negative or
 *         above its max is CS_ERR_INVALID, detected on the device and reported by this call; the tables are then undefined and
 *         the handle stays usable.
 * pred_table, truth_table: out, [batch][max][4] int32 {area, partner, overlap, n_major}, row l - 1 for label l, both
 *         table_kind; the row of a label that does not occur is all zeros.
 * n_pairs: out, host [batch], or NULL: the number of distinct pairs (p > 0, t > 0) with I > 0.
 * The pair counts live in an open-addressing table on the device, 12 bytes per slot.  params NULL or table_log2 0: its first
 * capacity is the power of two >= 2 * batch * (max_pred + max_truth), at least 2^16; else 2^table_log2, 10..26.  A table that
 * proves too small is doubled and the call runs again (cs_label_match_last_table counts the doublings); beyond 2^26 slots:
 * CS_ERR_NOMEM.  Every result is a sum, a maximum or a count of integers: bit-identical run to run, and independent of the
 * capacity and of the other images of the batch.  One host synchronisation per attempt.  Other bad arguments: CS_ERR_INVALID
 * before any device work; without a gfx950 device (p == NULL): CS_ERR_NO_DEVICE. */
typedef struct cs_match_params {
    int32_t table_log2;               /* 0: automatic; else 10..26: the first capacity */
    int32_t reserved;                 /* must be 0 */
} cs_match_params;
int cs_label_match(cs_preproc *p, const int32_t *pred, const int32_t *truth, int32_t batch, int32_t height, int32_t width,
                   int in_kind, int32_t max_pred, int32_t max_truth, const cs_match_params *params, int32_t *pred_table,
                   int32_t *truth_table, int table_kind, int64_t *n_pairs);
/* Device time of the last cs_label_match (its last attempt): clearing and the counting pass, and the reduction into the tables. */
int cs_label_match_last_timing(const cs_preproc *p, double *count_ms, double *reduce_ms);
/* The capacity (as log2) the last cs_label_match ended with, and how many times it doubled the table. */
int cs_label_match_last_table(const cs_preproc *p, int32_t *table_log2, int32_t *grows);

/* ---- growing labels by a distance ---------------------------------------------------------------- */
/* Every object of a label image grows outwards by sqrt(max_d2) pixels, and where two objects would meet each stops halfway
 * (tests/expand_reference.py restates the rule).  All integers, a function of the labels alone: with D2 the squared
 * Euclidean distance from a background pixel to the nearest pixel with a label > 0 of the same image (outside the image there
 * is nothing), a pixel with D2 <= max_d2 takes the label of that nearest pixel, the smallest label where several pixels of
 * different labels lie at that D2; labelled pixels keep their label, every other pixel stays 0, and no id is renumbered.  Off
 * the ties that is skimage.segmentation.expand_labels(labels, distance) with max_d2 the largest integer whose square root is
 * <= distance; the library's choice among equidistant pixels follows its scan order, this one the labels alone.
 * labels: [batch][height][width] int32, in_kind.  Left on the device by cs_segment_* on this handle they are read in stream
 *         order, as cs_extract_measure reads them.  height, width 1..4096, batch 1..65535 (above: CS_ERR_UNSUPPORTED).  A
 *         negative label is CS_ERR_INVALID, detected on the device and reported by this call; the outputs are then undefined
 *         and the handle stays usable.
 * params: not NULL; max_d2 1..16129 (distances up to 127 px), reserved 0.
 * out:    [batch][height][width] int32, out_kind; may be `labels` itself.
 * d2:     NULL, or [batch][height][width] uint16 where `out` is: 0 on labelled pixels, D2 where it is <= max_d2, 65535 elsewhere.
 * No atomics and no floating point: bit-identical run to run, and nothing crosses between the images of a batch.  Scratch
 * (5 bytes per pixel, and a host image's upload) comes from the buffers the handle's segmenter stages share.  One host
 * synchronisation per call.  Other bad arguments: CS_ERR_INVALID before any device work; without a gfx950 device (p == NULL):
 * CS_ERR_NO_DEVICE. */
typedef struct cs_expand_params { int32_t max_d2; /* 1..16129 */ int32_t reserved; /* 0 */ } cs_expand_params;
int cs_label_expand(cs_preproc *p, const int32_t *labels, int32_t batch, int32_t height, int32_t width, int in_kind,
                    const cs_expand_params *params, int32_t *out, uint16_t *d2 /* or NULL */, int out_kind);
/* Device time of the last cs_label_expand: the column pass (with the clearing of the status word) and the row pass. */
int cs_label_expand_last_timing(const cs_preproc *p, double *columns_ms, double *rows_ms);

/* ---- per-object intensities ------------------------------------------------------------------------- */
/* What every object of a label image measures in every channel of an image, as exact integer sums (DESIGN 3u;
 * tests/intensity_reference.py restates the rule).  An object is the set of pixels of one image with one label > 0, connected
 * or not, less the pixels where `exclude` is non-zero; r and c are the row and the column of a pixel in its image, v its value
 * in a channel.  scipy.ndimage.sum / mean / standard_deviation / minimum / maximum / center_of_mass over the labels, and
 * skimage.measure.regionprops' intensity properties, follow from the sums (cellscreen/intensity.py).
 * image:  [batch][height][width][channels] uint8 / uint16 (pixel_type), channels 1..4, every channel is measured; more than 4:
 *         CS_ERR_UNSUPPORTED (the caller splits the stack).
 * labels: [batch][height][width] int32, 0 = background.  Left on the device by cs_segment_* or cs_label_expand on this handle
 *         they are read in stream order.  A label that is negative or above max_label is CS_ERR_INVALID, detected on the device
 *         and reported by this call (whatever `exclude` holds there); it is never used as an index, the tables are then
 *         undefined and the handle stays usable.
 * exclude: NULL, or [batch][height][width] int32: a pixel whose value is non-zero, whatever the value, belongs to no object.
 *         With the nuclei as `exclude` under the grown cells as `labels` the objects are the rings of cytoplasm.
 * image, labels and exclude are all in_kind.  height, width 1..4096, batch 1..65535 (above: CS_ERR_UNSUPPORTED).
 * max_label: 1..2^20, an upper bound of the labels; it sizes the tables, row b * max_label + label - 1 for label `label` of
 *         image b.  Above 2^20, or batch * max_label * channels above 2^22: CS_ERR_UNSUPPORTED.
 * geom:   out, [batch][max_label][3] int64: area, sum r, sum c.
 * stats:  out, [batch][max_label][channels][6] int64: sum v, sum v^2, sum v * r, sum v * c, min v, max v.  Both out_kind.
 *         An object that does not occur, or that `exclude` covers whole, has all-zero rows, its minimum included.
 * No floating point: every result is a sum, a minimum or a maximum of integers, bit-identical run to run and independent of the
 * other images of the batch.  Uploads of host inputs and host tables on their way back go through the buffers the handle's
 * segmenter stages share.  One host synchronisation per call.  Other bad arguments: CS_ERR_INVALID before any device work;
 * without a gfx950 device (p == NULL): CS_ERR_NO_DEVICE. */
int cs_label_intensity(cs_preproc *p, const void *image, int pixel_type, int32_t channels,
                       const int32_t *labels, const int32_t *exclude /* or NULL */,
                       int32_t batch, int32_t height, int32_t width, int in_kind, int32_t max_label,
                       int64_t *geom, int64_t *stats, int out_kind);
/* Device time of the last cs_label_intensity: clearing the tables and the status word, and the pass with its closing step. */
int cs_label_intensity_last_timing(const cs_preproc *p, double *clear_ms, double *pass_ms);

/* ---- per-object median, quantiles and MAD ----------------------------------------------------------- */
/* Exact integer order statistics of every object of a label image in every channel of an image (DESIGN 3v;
 * tests/quantile_reference.py restates the rule).  The objects are cs_label_intensity's: the pixels of one image with one
 * label > 0, connected or not, less the pixels where `exclude` is non-zero.  A quantile is a rational num / den with
 * 0 <= num <= den and 1 <= den <= 65536.  For an object of n >= 1 pixels whose values in a channel, sorted, are s[0 .. n-1]:
 *     t = num * (n - 1)        (int64: below 2^40)
 *     lo = t / den,  rem = t % den,  hi = lo + (rem > 0)
 * The device writes s[lo] and s[hi]; the caller takes value = s[lo] + (s[hi] - s[lo]) * rem / den in float64, which is
 * numpy.quantile's method="linear"; s[lo] and s[hi] themselves are its "lower" and "higher".
 * With want_mad the device also takes the median's ranks (num / den = 1 / 2), m_lo and m_hi, then the doubled deviations
 * d = |2 v - (m_lo + m_hi)| (17 bits) and their order statistics d_lo, d_hi at the same two ranks.  median = (m_lo + m_hi) / 2
 * and MAD = (d_lo + d_hi) / 4 are exact in float64; no scale factor is applied (scipy.stats.median_abs_deviation, scale=1).
 * image, labels, exclude, in_kind, the sizes and max_label: as cs_label_intensity, a bad label included (CS_ERR_INVALID,
 *         detected on the device, whatever `exclude` holds there; the handle stays usable).
 * q_num, q_den: host arrays [n_q], n_q 1..8 (above: CS_ERR_UNSUPPORTED); duplicates and any order are kept.
 *         max_label above 2^20, or batch * max_label * channels * n_q above 2^22: CS_ERR_UNSUPPORTED.
 * count:  out, [batch][max_label] int32: the pixels of the object, row b * max_label + label - 1.
 * order:  out, [batch][max_label][channels][n_q][2] int32: s[lo], s[hi].
 * mad:    out, [batch][max_label][channels][4] int32: m_lo, m_hi, d_lo, d_hi; required iff want_mad.  All three out_kind.
 *         An object that does not occur, or that `exclude` covers whole, has all-zero rows.
 * No floating point on the device; bit-identical run to run and independent of the other images of the batch.  Besides the
 * buffers cs_label_intensity shares, the handle keeps 2 bytes per pixel and channel for the gathered values and 8 bytes per
 * row.  One host synchronisation per call.  Other bad arguments: CS_ERR_INVALID before any device work; without a gfx950
 * device (p == NULL): CS_ERR_NO_DEVICE. */
int cs_label_quantiles(cs_preproc *p, const void *image, int pixel_type, int32_t channels,
                       const int32_t *labels, const int32_t *exclude /* or NULL */,
                       int32_t batch, int32_t height, int32_t width, int in_kind, int32_t max_label,
                       const int32_t *q_num, const int32_t *q_den, int32_t n_q, int want_mad,
                       int32_t *count, int32_t *order, int32_t *mad /* or NULL */, int out_kind);
/* Device time of the last cs_label_quantiles: clearing + counting + offsets, the scatter into segments, the selection. */
int cs_label_quantiles_last_timing(const cs_preproc *p, double *count_ms, double *scatter_ms, double *select_ms);

/* ---- per-object Haralick texture -------------------------------------------------------------------- */
/* The grey-level co-occurrence matrices of every object of a label image in every channel of an image, reduced to exact
 * records from which Haralick's 13 features follow on the host (tests/texture_reference.py restates the rule).
 * The objects are cs_label_intensity's: the pixels of one image with one label > 0, connected or not, less the pixels where
 * `exclude` is non-zero.
 * Levels: per channel c a value v becomes q(v) = ((min(max(v, lo[c]), hi[c]) - lo[c]) * levels) / (hi[c] - lo[c] + 1), an
 *         integer division, exact for every value and span; 2 <= levels <= 64, 0 <= lo <= hi <= 65535.
 * Pairs:  one distance d, 1..127, and four directions k with the (row, column) steps (0, d), (d, d), (d, 0), (d, -d), the 2-D
 *         order of mahotas.  The pair (p, p + step_k) counts iff both pixels lie in the image, carry the same label > 0 and
 *         neither is excluded; it adds 1 to G[k][q(p)][q(p')] and 1 to G[k][q(p')][q(p)].  G is symmetric and its total N_k is
 *         twice the number of pairs, at most 2^25.  Pairs between objects or through an excluded pixel count nowhere.
 * image, labels, exclude, in_kind, the sizes and max_label: as cs_label_intensity, a bad label included (CS_ERR_INVALID,
 *         detected on the device, whatever `exclude` holds there; the handle stays usable).
 * range_lo, range_hi: host arrays [channels].
 * The rules apply in this order: those of cs_label_intensity up to its channel limit, then levels, distance and the ranges
 *         (CS_ERR_INVALID), then the caps (CS_ERR_UNSUPPORTED): max_label above 2^20, batch * max_label * channels * levels
 *         above 2^24, and with glcm batch * max_label * channels * levels^2 above 2^24; then the limits of the image.
 * count:  out, [batch][max_label] int32: the pixels of the object, row b * max_label + label - 1.
 * marg:   out, [batch][max_label][channels][4][4 * levels] int32, per direction: the row marginal px[i] = sum_j G[i][j]
 *         (levels entries), the sum marginal ps[s] = sum over i + j = s (2 * levels - 1 entries and one zero), the difference
 *         marginal pd[t] = sum over |i - j| = t (levels entries).  N_k = sum px.
 * sumsq:  out, [batch][max_label][channels][4] int64: sum of G^2.
 * clogc:  out, [batch][max_label][channels][4] double: sum over the cells with G > 0 of G * log2(G), the one value that is not
 *         an integer; summed in a fixed order, so bit-identical run to run.  The joint entropy is log2(N) - clogc / N.
 * glcm:   out or NULL, [batch][max_label][channels][4][levels][levels] int32: the matrices themselves.  All five out_kind.
 *         An object that does not occur, or that `exclude` covers whole, has all-zero rows, as has a direction without pairs.
 * Bit-identical run to run and independent of the other images of the batch.  Besides the buffers cs_label_intensity shares,
 * the handle keeps 16 bytes per row for the bounding boxes.  One host synchronisation per call.  Other bad arguments:
 * CS_ERR_INVALID before any device work; without a gfx950 device (p == NULL): CS_ERR_NO_DEVICE. */
int cs_label_texture(cs_preproc *p, const void *image, int pixel_type, int32_t channels,
                     const int32_t *labels, const int32_t *exclude /* or NULL */,
                     int32_t batch, int32_t height, int32_t width, int in_kind, int32_t max_label,
                     int32_t levels, int32_t distance, const int32_t *range_lo, const int32_t *range_hi,
                     int32_t *count, int32_t *marg, int64_t *sumsq, double *clogc, int32_t *glcm /* or NULL */, int out_kind);
/* Device time of the last cs_label_texture: clearing + the boxes, and the matrices with their reduction. */
int cs_label_texture_last_timing(const cs_preproc *p, double *boxes_ms, double *matrices_ms);

/* ---- per-object size and shape ------------------------------------------------------------------------ */
/* The geometry of every object of a label image as exact integer records, from which the host derives area, bounding box, extent,
 * centroid, central moments, inertia tensor, axis lengths, eccentricity, orientation, Hu's moments, perimeter, form factor, Euler
 * numbers, convex area, solidity and Feret diameters (tests/shape_reference.py restates the rule, cellscreen/shape.py
 * derives).  The objects are cs_label_intensity's: the pixels of one image with one label > 0, connected or not, less the pixels
 * where `exclude` is non-zero.  Let e be the effective plane: the label, or 0 where excluded or outside the image.  Everything
 * below is a function of e alone; no image is read.  Per (image b, label L), row b * max_label + L - 1:
 * moments: out, [batch][max_label][10] int64: n, sum r, sum c, sum r^2, sum rc, sum c^2, sum r^3, sum r^2 c, sum r c^2, sum c^3
 *         over the pixels (r, c) of the object, image coordinates.  One label over a 4096 x 4096 plane keeps every sum below 2^59.
 * box:    out, [batch][max_label][4] int32: minr, minc, maxr, maxc, the max exclusive (regionprops' bbox).
 * quads:  out, [batch][max_label][16] int32: the histogram of the 2 x 2 bit quads over the (H + 1) (W + 1) corner positions of the
 *         plane padded by one background pixel, the code [e(r,c)==L] + 2 [e(r+1,c)==L] + 4 [e(r,c+1)==L] + 8 [e(r+1,c+1)==L] for
 *         r = -1 .. H-1 and c = -1 .. W-1; bin 0 is left zero.  Gray's counts are Q1 (one bit set), Q3 (three) and QD (codes 6 and
 *         9); the Euler number is (Q1 - Q3 + 2 QD) / 4 for 4-connectivity and (Q1 - Q3 - 2 QD) / 4 for 8-connectivity.
 * perim:  out, [batch][max_label][3] int32: the three classes of skimage.measure.perimeter(mask, neighbourhood=4).  A border pixel
 *         is a pixel of the object with a 4-neighbour that is not the object's, outside the image included.  For a border pixel a
 *         is the number of its 4-neighbours that are border pixels of the same object and d that of its diagonal neighbours; the
 *         value 1 + 2a + 10d counts in class 0 if it is one of {5, 7, 15, 17, 25, 27}, in class 1 if one of {21, 33}, in class 2 if
 *         one of {13, 23}.  perimeter = n0 + n1 sqrt(2) + n2 (1 + sqrt(2)) / 2.  Neighbouring objects are background to each other.
 * hull:   out, [batch][max_label][4] int64, required iff want_hull (else NULL): convex_area, feret_max2, feret_min_num,
 *         feret_min_den.  The hull is that of the pixel-edge midpoints (2r +- 1, 2c), (2r, 2c +- 1) of the object's pixels in
 *         doubled coordinates, the one cs_extract_measure builds.  convex_area counts the pixel centres inside or on it.  feret_max2
 *         is the largest squared distance between two of its vertices: the diameter is sqrt(feret_max2) / 2.  Every edge (a, b) of
 *         the hull has the width w = max over the vertices v of |cross(b - a, v - a)|; the edge with the smallest w^2 / |b - a|^2,
 *         among equal quotients the one with the smaller |b - a|^2, gives feret_min_num = w and feret_min_den = |b - a|^2: the
 *         diameter is w / (2 sqrt(den)).  This is the width of the object's own hull; scikit-image's feret_diameter_max traces the
 *         contour of the convex image instead, a deliberate difference.
 * labels, exclude, in_kind, the sizes and max_label: as cs_label_intensity, a bad label included (CS_ERR_INVALID "negative or
 *         exceeds max_label", detected on the device, whatever `exclude` holds there; the handle stays usable).
 * The rules apply in cs_label_intensity's order: NULL arguments and hull against want_hull, the memory kinds, the sizes, max_label
 *         (CS_ERR_INVALID), then the caps (CS_ERR_UNSUPPORTED): max_label above 2^20, batch * max_label above 2^22; then the
 *         limits of the image.  All five out_kind.  An object that does not occur, or that `exclude` covers whole, has all-zero
 *         rows.
 * No floating point on the device; bit-identical run to run and independent of the other images of the batch.  The handle shares
 * cs_label_intensity's buffers and cs_label_texture's 16 bytes per row for the bounding boxes.  One host synchronisation per call.
 * Other bad arguments: CS_ERR_INVALID before any device work; without a gfx950 device (p == NULL): CS_ERR_NO_DEVICE. */
int cs_label_shape(cs_preproc *p, const int32_t *labels, const int32_t *exclude /* or NULL */,
                   int32_t batch, int32_t height, int32_t width, int in_kind, int32_t max_label, int want_hull,
                   int64_t *moments, int32_t *box, int32_t *quads, int32_t *perim, int64_t *hull /* or NULL */, int out_kind);
/* Device time of the last cs_label_shape: clearing + the moments and boxes, and the outline pass (quads, perimeter, hull). */
int cs_label_shape_last_timing(const cs_preproc *p, double *moments_ms, double *outline_ms);

/* ---- per-object neighbours and contact --------------------------------------------------------------- */
/* Who lies near every object of a label image, and how much of its outline is in contact, as exact integer records (DESIGN 3y;
 * tests/neighbors_reference.py restates the rule, cellscreen/neighbors.py derives).  The objects are cs_label_intensity's without an
 * `exclude` plane: the pixels of one image with one label > 0, connected or not.  Nothing crosses between the images of a batch, and
 * outside the image there is nothing.  Distances are squared Euclidean distances between pixel centres, in integers.
 *   A border pixel of a is a pixel of a with a 4-neighbour that is not a's, outside the image included (cs_label_shape's rule).
 *   D2(a, b), a != b, is the smallest squared distance between a pixel of a and a pixel of b; b is a neighbour of a iff
 *         D2(a, b) <= max_d2, whatever lies between them: CellProfiler's dilation of a by strel_disk(d) with max_d2 = d * d.
 *   A border pixel of a is touching iff a pixel with a label other than 0 and a lies within max_d2 of it; its nearest foreign label
 *         is the label of that pixel at the smallest (d2, label).
 * params: not NULL.  max_d2 1..1024 (1: 4-adjacent, 2: 8-adjacent; distances up to 32 px, above: CS_ERR_UNSUPPORTED); table_log2 0
 *         (automatic) or 10..26: the first capacity of the pair table; reserved 0.
 * geom:   out, [batch][max_label][3] int64: area, sum r, sum c -- cs_label_intensity's geom, bit for bit.
 * objects: out, [batch][max_label][3] int32: border, touching, degree (the number of neighbours); all zero for a label that does
 *         not occur.
 * offsets: out, [batch * max_label + 1] int64: the CSR row starts, row b * max_label + l - 1 for label l of image b; the last entry
 *         is the number of directed pairs.  All three out_kind.
 * n_pairs: out, host, not NULL: that number.
 * The pairs stay on the handle until the next cs_label_neighbors: [n_pairs][3] int32 {neighbour label, D2(a, b), n_near}, every row
 *         sorted by neighbour label whatever its length.  n_near is the number of a's border pixels whose nearest foreign label is
 *         that neighbour (it may be 0); the n_near of a row sum to a's touching.  cs_label_neighbors_pairs copies them out.
 * labels, in_kind, the sizes and max_label: as cs_label_intensity, a bad label included (CS_ERR_INVALID "negative or exceeds
 *         max_label", detected on the device, never an index or a key; the handle stays usable).
 * The rules apply in cs_label_intensity's order: NULL arguments, the memory kinds, the sizes, max_label, max_d2 < 1, reserved,
 *         table_log2 (CS_ERR_INVALID), then the caps (CS_ERR_UNSUPPORTED): sides above 4096, batch above 65535, max_label above 2^20,
 *         batch * max_label above 2^22, max_d2 above 1024.
 * The pairs are collected in an open-addressing table on the device, 16 bytes per slot, and leave through 28 more bytes per slot.
 *         Automatic: the power of two >= 8 * batch * max_label, 2^16 to 2^24.  A table that proves too small is doubled and the call
 *         runs again (cs_label_neighbors_last_table counts the doublings); beyond 2^26 slots: CS_ERR_NOMEM.
 * No floating point on the device.  Every value is a count, a minimum or a sum of integers: bit-identical run to run, independent of
 * the capacity, of the slot placement and of the other images of the batch.  Scratch comes from the buffers the handle's segmenter
 * stages share.  One host synchronisation per attempt.  Other bad arguments: CS_ERR_INVALID before any device work; without a gfx950
 * device (p == NULL): CS_ERR_NO_DEVICE. */
typedef struct cs_neighbors_params {
    int32_t max_d2;                   /* 1..1024 */
    int32_t table_log2;               /* 0: automatic; else 10..26: the first capacity */
    int32_t reserved;                 /* must be 0 */
} cs_neighbors_params;
int cs_label_neighbors(cs_preproc *p, const int32_t *labels, int32_t batch, int32_t height, int32_t width, int in_kind,
                       int32_t max_label, const cs_neighbors_params *params, int64_t *geom, int32_t *objects, int64_t *offsets,
                       int out_kind, int64_t *n_pairs);
/* The pair list of the last successful cs_label_neighbors on this handle into pairs, [capacity][3] int32, pairs_kind.  Without such a
 * call, or with a capacity below its n_pairs: CS_ERR_INVALID.  One host synchronisation. */
int cs_label_neighbors_pairs(cs_preproc *p, int32_t *pairs, int64_t capacity, int pairs_kind);
/* Device time of the last cs_label_neighbors (its last attempt): clearing + the scan of the disks, and the rows (degrees, offsets,
 * scatter, sort). */
int cs_label_neighbors_last_timing(const cs_preproc *p, double *scan_ms, double *rows_ms);
/* The capacity (as log2) the last cs_label_neighbors ended with, and how many times it doubled the table. */
int cs_label_neighbors_last_table(const cs_preproc *p, int32_t *table_log2, int32_t *grows);

/* ---- per-object colocalization between channels ------------------------------------------------------ */
/* How the channels of an image go together inside every object of a label image, as exact integer sums (DESIGN 3z;
 * tests/colocalize_reference.py restates the rule, cellscreen/colocalize.py derives).  The objects are cs_label_intensity's: the
 * pixels of one image with one label > 0, connected or not, less the pixels where `exclude` is non-zero.  The pairs of channels
 * (i, j), i < j, come in lexicographic order: P = channels * (channels - 1) / 2.  Pearson's correlation and the regression slope
 * (scipy.stats.pearsonr, linregress), Manders' M1 / M2, the overlap coefficient, K1 / K2 and the rank-weighted coefficients of
 * CellProfiler's MeasureColocalization follow from the sums on the host.
 * A pixel of an object is "above" in channel c
 *   absolute == 0:  iff v * thr_den >= thr_num * max_c, max_c the object's own maximum in c; 0 <= thr_num <= thr_den, thr_den in
 *                   1..65536.  A tie is above.
 *   absolute == 1:  iff v >= abs_thr[c], each 0..65536.
 * and "both" of a pair where it is above in both channels.  With rwc, per image and channel, the dense rank of a value among the
 * values that occur on the image's object pixels (0 upwards; R_c distinct values), and per pair R = max(R_i, R_j),
 * w = R - |rank_i - rank_j| in 1..65536.
 * image:  [batch][height][width][channels] uint8 / uint16 (pixel_type), channels 2..4; 1: CS_ERR_INVALID, above 4:
 *         CS_ERR_UNSUPPORTED.
 * labels, exclude, in_kind, the sizes and max_label: as cs_label_intensity, a bad label included (CS_ERR_INVALID "negative or
 *         exceeds max_label", detected on the device, never an index; the handle stays usable).
 * geom:   out, [batch][max_label][3] int64: area, sum r, sum c -- cs_label_intensity's geom, bit for bit.
 * chan:   out, [batch][max_label][channels][5] int64: sum v, sum v^2, max v, n_above, sum v[above].
 * pair:   out, [batch][max_label][P][9] int64: sum v_i v_j over all pixels; over "both": n, sum v_i, sum v_j, sum v_i^2,
 *         sum v_j^2, sum v_i v_j, sum v_i w, sum v_j w (the last two zero when rwc == 0).
 * levels: out, [batch][channels] int32: R_c; zeros when rwc == 0.  All four out_kind.  Rows of absent objects are all zero.
 * The rules apply in cs_label_intensity's order, the parameters' ranges (CS_ERR_INVALID) after the channel limit.  With rwc the
 * handle keeps 192 KB per image and channel for the presence and rank tables; above 1 GiB: CS_ERR_UNSUPPORTED (split the batch),
 * before any device work.  No floating point: bit-identical run to run and independent of the other images of the batch.  One
 * host synchronisation per call.  Without a gfx950 device (p == NULL): CS_ERR_NO_DEVICE. */
typedef struct cs_colocalize_params {
    int32_t thr_num, thr_den;         /* used when absolute == 0 */
    int32_t absolute;                 /* 0 / 1 */
    int32_t abs_thr[4];               /* used when absolute == 1 */
    int32_t rwc;                      /* 0 / 1 */
} cs_colocalize_params;
int cs_label_colocalize(cs_preproc *p, const void *image, int pixel_type, int32_t channels,
                        const int32_t *labels, const int32_t *exclude /* or NULL */,
                        int32_t batch, int32_t height, int32_t width, int in_kind, int32_t max_label,
                        const cs_colocalize_params *params, int64_t *geom, int64_t *chan, int64_t *pair, int32_t *levels,
                        int out_kind);
/* Device time of the last cs_label_colocalize: clearing, the moments walk, the ranks (0 without rwc) and the thresholded walk. */
int cs_label_colocalize_last_timing(const cs_preproc *p, double *clear_ms, double *moments_ms, double *ranks_ms,
                                    double *thresholded_ms);

/* ---- per-object radial intensity distribution and edge intensities ------------------------------------ */
/* Where the intensity of every object of a label image sits between its centre and its outline, and how bright its outline is, as
 * exact integer records (tests/radial_reference.py restates the rule, cellscreen/radial.py derives): CellProfiler's
 * MeasureObjectIntensityDistribution (FracAtD, MeanFrac, RadialCV per ring) and the Edge measures of MeasureObjectIntensity.  The
 * objects are cs_label_intensity's: the pixels of one image with one label > 0, connected or not, less the pixels where `exclude`
 * is non-zero; a pixel's effective label is 0 where `exclude` is set.  Nothing crosses between the images of a batch.
 *   E2(p), the depth of an object pixel p: the smallest squared Euclidean distance between pixel centres from p to a position that
 *         is not the object's: a pixel of another label, background, an excluded pixel, or any position outside the image.  E2 == 1
 *         exactly on the border pixels of cs_label_shape and cs_label_neighbors; per object it is
 *         scipy.ndimage.distance_transform_edt(np.pad(labels == l, 1)) ** 2.  Depths are exact up to CS_RADIAL_MAX_D2 = 127^2: an
 *         object with a deeper pixel is CS_ERR_UNSUPPORTED, detected on the device as a bad label is; the handle stays usable.
 *   The centre of an object is its deepest pixel, among equally deep ones the one with the smallest raster index r * width + c
 *         (scipy.ndimage.maximum_position), or the caller's.  C2(p) is the squared Euclidean distance from p to the centre along
 *         the straight line; CellProfiler propagates that distance inside the object instead, a deliberate difference: the two
 *         agree wherever the segment from p to the centre stays inside the object.
 *   ring(p), with B = bins: the number of k in 1..B-1 with (B - k)^2 * C2 >= k^2 * E2, in 64-bit integers: floor(B dc / (dc + de))
 *         with dc = sqrt(C2), de = sqrt(E2), decided without a root; an exact multiple belongs to the outer ring, the centre to
 *         ring 0.
 *   wedge(p) = (r > rc) + 2 * (c > cc) + 4 * (|r - rc| > |c - cc|) around the centre (rc, cc): CellProfiler's eight.
 * image, pixel_type, channels 1..4, labels, exclude, in_kind, the sizes and max_label: as cs_label_intensity, a bad label included
 *         (CS_ERR_INVALID "negative or exceeds max_label", detected on the device, never an index or a key; the handle stays usable).
 * params: not NULL.  bins 1..CS_RADIAL_MAX_BINS (below 1: CS_ERR_INVALID, above: CS_ERR_UNSUPPORTED); reserved 0.
 * centers: NULL, or a HOST table [batch][max_label][2] int32 of rows and columns, whatever in_kind: every row, those of absent
 *         objects too, must lie inside the image (else CS_ERR_INVALID before any device work).  A centre need not lie in its object.
 * geom:   out, [batch][max_label][3] int64: area, sum r, sum c -- cs_label_intensity's geom, bit for bit.
 * center: out, [batch][max_label][4] int32: the centre's row and column, E2 at the object's deepest pixel (also with given
 *         centres), the number of pixels with E2 == 1.
 * ring:   out, [batch][max_label][bins][8][1 + channels] int64: per (object, ring, wedge) the pixel count and per channel sum v.
 * edge:   out, [batch][max_label][channels][4] int64: sum v, sum v^2, min v, max v over the pixels with E2 == 1.
 * d2:     out or NULL, [batch][height][width] uint16: E2, 0 off the objects.  All five out_kind.  Rows of absent objects are all
 *         zero.
 * The rules apply in cs_label_intensity's order, the parameters' ranges after the channel limit; then the caps (CS_ERR_UNSUPPORTED):
 *         max_label above 2^20, batch * max_label * channels above 2^22, sides above 4096, batch above 65535, a ring table above
 *         1 GiB (split the batch); then the centres.
 * No floating point: bit-identical run to run and independent of the other images of the batch.  Scratch comes from the buffers the
 * handle's stages share (1 byte per pixel of column distances, 2 of depths, 8 per table row); the handle keeps nothing beyond them.
 * One host synchronisation per call.  Without a gfx950 device (p == NULL): CS_ERR_NO_DEVICE. */
#define CS_RADIAL_MAX_D2 16129        /* 127^2: the deepest E2 an object may hold */
#define CS_RADIAL_MAX_BINS 16
typedef struct cs_radial_params {
    int32_t bins;                     /* 1..CS_RADIAL_MAX_BINS */
    int32_t reserved;                 /* must be 0 */
} cs_radial_params;
int cs_label_radial(cs_preproc *p, const void *image, int pixel_type, int32_t channels,
                    const int32_t *labels, const int32_t *exclude /* or NULL */,
                    int32_t batch, int32_t height, int32_t width, int in_kind, int32_t max_label,
                    const cs_radial_params *params, const int32_t *centers /* or NULL */,
                    int64_t *geom, int32_t *center, int64_t *ring, int64_t *edge, uint16_t *d2 /* or NULL */, int out_kind);
/* Device time of the last cs_label_radial: clearing + the column pass, the row pass with the centres, and the bin pass. */
int cs_label_radial_last_timing(const cs_preproc *p, double *columns_ms, double *rows_ms, double *bins_ms);

/* ---- per-object granularity spectrum --------------------------------------------------------------------- */
/* The size spectrum of the bright structures inside every object of a label image, as exact integer records (DESIGN 3zb;
 * tests/granularity_reference.py restates the rule, cellscreen/granularity.py derives): CellProfiler's MeasureGranularity.  The
 * objects are cs_label_intensity's: the pixels of one image with one label > 0, connected or not, less the pixels where `exclude`
 * is non-zero; a pixel's effective label is 0 where `exclude` is set.  Nothing crosses between the images of a batch or between
 * channels.
 *   P, the working plane of a channel: uint16 [Hs][Ws], Hs = ceil(height / s), Ws = ceil(width / s), s = subsample.
 *         P[R][C] = (2 * sum v + n) / (2 * n) (integer division) over the in-image pixels of the s x s block, n their count: the
 *         rounded block mean, the pixel itself at s = 1; uint8 is widened.  With masked = 1 a pixel whose effective label is 0
 *         contributes v = 0 and still counts in n (CellProfiler with the objects as the image's mask).
 *   E_k = the erosion of E_(k-1) by the 3 x 3 cross (CellProfiler's disk(1)), E_0 = P; neighbours outside the plane are ignored:
 *         scipy.ndimage.grey_erosion(E, footprint=cross, mode='reflect').
 *   R_k = the reconstruction by dilation of E_k under P with the same cross: the fixed point of
 *         R <- min(max over the cross of R, P) started at R = E_k, neighbours outside ignored; R_0 = P.  k = 1..steps.
 * Deliberate differences from CellProfiler: the subsampling is an integer block mean read back by the nearest block (CellProfiler:
 * bilinear map_coordinates); there is no background removal (pass a plane corrected by cs_segment_background); the reconstruction
 * is image-wide, so a bright structure shared by two touching objects is held up for both, as in CellProfiler.
 * image, pixel_type, channels 1..4, labels, exclude, in_kind, the sizes and max_label: as cs_label_intensity, a bad label included
 *         (CS_ERR_INVALID "negative or exceeds max_label", detected on the device, never an index or a key; the handle stays usable).
 * params: not NULL.  steps 1..CS_GRANULARITY_MAX_STEPS (below 1: CS_ERR_INVALID, above: CS_ERR_UNSUPPORTED); subsample 1, 2, 4 or
 *         8, masked 0 or 1, reserved 0 (else CS_ERR_INVALID).
 * geom:   out, [batch][max_label][3] int64: area, sum r, sum c -- cs_label_intensity's geom, bit for bit.
 * sums:   out, [batch][max_label][steps + 1][channels] int64: for k = 0..steps the sum over the object's full-resolution pixels
 *         (r, c) of R_k[r / s][c / s].
 * image_sums: out, [batch][steps + 1][channels] int64: the sum over the whole working plane of R_k (CellProfiler's image-level
 *         Granularity_k follows from it).
 * planes: out or NULL, uint16 [batch][steps + 1][channels][Hs][Ws]: the R_k themselves.  All four out_kind.  Rows of absent
 *         objects are all zero.
 * The rules apply in cs_label_intensity's order, the parameters' ranges after the channel limit; then the caps (CS_ERR_UNSUPPORTED):
 *         max_label above 2^20, batch * max_label * channels above 2^22, sides above 4096, batch above 65535, a sums table or a
 *         planes stack above 1 GiB (split the batch).  A refused call writes nothing.
 * The reconstruction runs in rounds over tiles until a round changes nothing, at most Hs * Ws rounds per step: reaching that cap
 * is CS_ERR_UNSUPPORTED, never an endless loop.  No floating point: bit-identical run to run and independent of the other images of
 * the batch.  Scratch comes from the buffers the handle's stages share (three uint16 working planes per channel, 4 bytes per
 * 64 x 32 tile of them, the control words, the tables on their way to the host); the handle keeps nothing beyond them.  A bad label
 * ends the call at its first read of the control word, before the tables are written.  One host synchronisation per group of rounds.
 * Without a gfx950 device (p == NULL): CS_ERR_NO_DEVICE. */
#define CS_GRANULARITY_MAX_STEPS 64
typedef struct cs_granularity_params {
    int32_t steps;                    /* 1..CS_GRANULARITY_MAX_STEPS */
    int32_t subsample;                /* 1, 2, 4 or 8 */
    int32_t masked;                   /* 0, or 1: pixels off the objects count as 0 in P */
    int32_t reserved;                 /* must be 0 */
} cs_granularity_params;
int cs_label_granularity(cs_preproc *p, const void *image, int pixel_type, int32_t channels,
                         const int32_t *labels, const int32_t *exclude /* or NULL */,
                         int32_t batch, int32_t height, int32_t width, int in_kind, int32_t max_label,
                         const cs_granularity_params *params,
                         int64_t *geom, int64_t *sums, int64_t *image_sums, uint16_t *planes /* or NULL */, int out_kind);
/* Device time of the last cs_label_granularity: clearing + the working planes, the erosions with their reconstructions, and the
 * sums passes (steps + 1 of them). */
int cs_label_granularity_last_timing(const cs_preproc *p, double *prepare_ms, double *steps_ms, double *sums_ms);
/* The reconstruction rounds of the last cs_label_granularity, all steps together, and its reads of the control word (one host
 * synchronisation each); either pointer may be NULL. */
int cs_label_granularity_last_rounds(const cs_preproc *p, int32_t *rounds, int32_t *reads);

/* ---- growing labels inside a mask by geodesic cost ------------------------------------------------------- */
/* The seeds of a label image grow inside a mask along the cheapest paths (tests/propagate_reference.py restates the
 * rule): CellProfiler's IdentifySecondaryObjects "Propagation" / "Watershed - Image", skimage.segmentation.watershed(guide, markers,
 * mask=) with an explicit cost.  All integers, per image of the batch:
 *   A seed pixel (seeds > 0) is a source: cost 0, it keeps its label whatever the mask says, is never relabelled and is never
 *   entered by a path.  A path starts at a seed pixel and then moves only through pixels that are no seed and whose mask is
 *   non-zero, to 4- or 8-neighbours inside the image.  A step q -> p costs lam * w + |g(p) - g(q)|: w by the metric
 *   (CS_PROPAGATE_CITYBLOCK: 1, 4-neighbours; _CHESSBOARD: 1, 8-neighbours; _CHAMFER: 5 axial and 7 diagonal, 8-neighbours), g
 *   the guide's channel (the term is 0 without a guide).  A candidate whose cost exceeds max_cost is not taken.  The key of a
 *   pixel is the lexicographic minimum over all such paths of (cost, label of the path's seed): the smallest cost, and among the
 *   labels that reach it at that cost the smallest.  A pixel that no path reaches keeps label 0 and cost -1.
 * Deliberate differences from CellProfiler's Propagation: the geometric and the intensity term add (there: under a square root);
 * the intensity term is the difference of two pixels (there: of 3 x 3 neighbourhoods); lam >= 1, so there is no pure-intensity
 * limit; a tie goes to the smallest label.
 * seeds:  [batch][height][width] int32, in_kind, 0 = background, labels 1..2^20.  Left on the device by cs_segment_* on this handle
 *         they are read in stream order.  A negative seed or one above 2^20 is CS_ERR_INVALID, detected on the device before it
 *         is a key and reported by this call; `out` is then undefined and the handle stays usable.  height, width 1..4096, batch
 *         1..65535, and batch * height * width * 8 bytes of keys at most 1 GiB (above: CS_ERR_UNSUPPORTED, split the batch).
 * mask:   NULL (everywhere), or [batch][height][width] uint8 where `seeds` is, non-zero = may be grown into.
 * guide:  NULL, or [batch][height][width][guide_channels] of guide_pixel_type (CS_PIX_U8 / CS_PIX_U16) where `seeds` is,
 *         guide_channels 1..4, cs_label_intensity's layout; params->guide_channel picks the channel.  Without a guide
 *         guide_channels and guide_pixel_type are not read and guide_channel must be 0.
 * params: not NULL; lam 1..255, max_cost 1..CS_PROPAGATE_NO_LIMIT (CS_PROPAGATE_NO_LIMIT = 2^40 - 2: no limit), reserved 0.
 * out:    [batch][height][width] int32, out_kind; may be `seeds` itself.
 * cost:   NULL, or [batch][height][width] int64 where `out` is: 0 on seeds, the cost where a path reached, -1 elsewhere.
 * The keys are the least fixed point of K(p) = min(K(p), min over q of K(q) + step(q, p)); the device relaxes 64 x 16 tiles in
 * rounds until a round changes nothing, only the tiles at the moving front after the first round, at most height * width rounds
 * that change something: reaching that cap is CS_ERR_UNSUPPORTED, never an endless loop.  The cost of a call grows with the winding
 * of the mask, one round per tile crossing.  No floating point, atomics only on the control words: the result is bit-identical
 * run to run and nothing crosses between the images of a batch.  Scratch (8 + 1 bytes per pixel, 2 more with a guide, 4 per tile,
 * and the uploads of host planes) comes from the buffers the handle's segmenter stages share.  One host synchronisation per group
 * of rounds (8, 16, 32, then 64 rounds).  Other bad arguments: CS_ERR_INVALID before any device work; without a gfx950 device
 * (p == NULL): CS_ERR_NO_DEVICE. */
#define CS_PROPAGATE_CITYBLOCK 0
#define CS_PROPAGATE_CHESSBOARD 1
#define CS_PROPAGATE_CHAMFER 2
#define CS_PROPAGATE_NO_LIMIT 1099511627774LL
typedef struct cs_propagate_params {
    int32_t metric;                   /* CS_PROPAGATE_* */
    int32_t lam;                      /* 1..255 */
    int32_t guide_channel;            /* 0..guide_channels - 1; 0 without a guide */
    int32_t reserved;                 /* must be 0 */
    int64_t max_cost;                 /* 1..CS_PROPAGATE_NO_LIMIT */
} cs_propagate_params;
int cs_label_propagate(cs_preproc *p, const int32_t *seeds, int32_t batch, int32_t height, int32_t width, int in_kind,
                       const uint8_t *mask /* or NULL */, const void *guide /* or NULL */, int32_t guide_channels, int guide_pixel_type,
                       const cs_propagate_params *params, int32_t *out, int64_t *cost /* or NULL */, int out_kind);
/* Device time of the last cs_label_propagate: clearing + the key plane, the rounds, and the labels' pass; and the number of rounds
 * (the closing quiet one included).  Any pointer may be NULL. */
int cs_label_propagate_last_timing(const cs_preproc *p, double *init_ms, double *relax_ms, double *finish_ms, int32_t *rounds);

/* ---- image and per-object focus and saturation records ---------------------------------------------------- */
/* Whether an image is worth measuring, as exact integer records (tests/quality_reference.py restates the rule,
 * cellscreen/quality.py derives): CellProfiler's MeasureImageQuality.  Every channel x of an image [height][width] is measured on
 * its own.  A pixel (r, c) is interior iff 1 <= r <= height - 2 and 1 <= c <= width - 2: there is no reflection and no padding, a
 * pixel without a full 3 x 3 neighbourhood has no focus value, and an image with a side below 3 has n_int = 0.  At an interior pixel
 *   L  = x[r-1][c] + x[r+1][c] + x[r][c-1] + x[r][c+1] - 4 x[r][c]       (scipy.ndimage.laplace, cv2.Laplacian(ksize=1))
 *   G  = gx^2 + gy^2, gx and gy the 3 x 3 Sobel responses, weights 1-2-1 (Tenengrad; scipy.ndimage.sobel along each axis)
 *   Br = (x[r][c+1] - x[r][c-1])^2 + (x[r+1][c] - x[r-1][c])^2           (Brenner's gradient, centred)
 * image:  [batch][height][width][channels] uint8 / uint16 (pixel_type), in_kind, channels 1..4 (more: CS_ERR_UNSUPPORTED).
 *         height, width 1..4096, batch 1..65535 (above: CS_ERR_UNSUPPORTED).
 * tile:   0: no mesh, or 16..1024 (else CS_ERR_INVALID): a mesh of m_r = ceil(height / tile) by m_c = ceil(width / tile) tiles,
 *         pixel (r, c) in tile ((r * m_r) / height, (c * m_c) / width) (integer division; CellProfiler's LocalFocusScore grid).
 *         batch * channels * m_r * m_c above 2^20: CS_ERR_UNSUPPORTED.
 * sat_level: NULL (the top of the pixel type: 255 / 65535), or [channels] int32 on the host, each 0..65536 (else CS_ERR_INVALID).
 * records: out, [batch][channels][CS_QUALITY_RECORD] int64: n, sum v, sum v^2, min, max, n_at_min, n_at_max (the pixels equal to
 *         the image's own minimum / maximum in that channel), n_sat (v >= sat_level), n_int, sum L, sum L^2, sum G, sum Br.
 * mesh:   with tile > 0 out, [batch][channels][m_r][m_c][CS_QUALITY_TILE] int64: n, sum v, sum v^2, n_int, sum L, sum L^2, sum G,
 *         sum Br of the tile's pixels; the stencil reads across tile borders, a pixel's values go to the tile that holds the pixel,
 *         and the tile records of an image sum to its record.  With tile == 0 it is not written and may be NULL.  Both out_kind.
 * At 4096 x 4096 uint16 sum L^2 <= (4 * 65535)^2 * 2^24 < 1.16e18 and sum G <= twice that, below 2^63.  No floating point and no
 * float atomics: bit-identical run to run and independent of the other images of the batch.  Uploads, the tables on their way to
 * the host and the workgroups' partial extremes go through the buffers the handle's segmenter stages share.  One host
 * synchronisation per call.  Other bad arguments: CS_ERR_INVALID before any device work; without a gfx950 device (p == NULL):
 * CS_ERR_NO_DEVICE. */
#define CS_QUALITY_RECORD 13
#define CS_QUALITY_TILE 8
#define CS_QUALITY_FOCUS 5
int cs_image_quality(cs_preproc *p, const void *image, int pixel_type, int32_t channels,
                     int32_t batch, int32_t height, int32_t width, int in_kind, int32_t tile,
                     const int32_t *sat_level /* or NULL */, int64_t *records, int64_t *mesh /* or NULL */, int out_kind);
/* Device time of the last cs_image_quality: clearing the tables, and the pass with its closing step. */
int cs_image_quality_last_timing(const cs_preproc *p, double *clear_ms, double *pass_ms);
/* The same focus values per object of a label image.  The objects are cs_label_intensity's: the pixels of one image with one
 * label > 0, connected or not, less the pixels where `exclude` is non-zero.  The stencil reads the image, not the labels, so the
 * sharpness of an object's own edge counts; a pixel of an object has focus values iff it is interior to the IMAGE.
 * image, pixel_type, channels 1..4, labels, exclude, in_kind, the sizes and max_label: as cs_label_intensity, a bad label included
 *         (CS_ERR_INVALID "negative or exceeds max_label", detected on the device, never an index or a key; the handle stays usable).
 * geom:   out, [batch][max_label][3] int64: area, sum r, sum c -- cs_label_intensity's geom, bit for bit.
 * focus:  out, [batch][max_label][channels][CS_QUALITY_FOCUS] int64: n_int, sum L, sum L^2, sum G, sum Br over the object's
 *         interior pixels.  Both out_kind; rows of absent objects are all zero.
 * The rules and the caps are cs_label_intensity's, in its order.  No floating point; bit-identical run to run and independent of
 * the other images of the batch; scratch from the shared buffers only; one host synchronisation per call. */
int cs_object_focus(cs_preproc *p, const void *image, int pixel_type, int32_t channels,
                    const int32_t *labels, const int32_t *exclude /* or NULL */,
                    int32_t batch, int32_t height, int32_t width, int in_kind, int32_t max_label,
                    int64_t *geom, int64_t *focus, int out_kind);
/* Device time of the last cs_object_focus: clearing the tables and the status word, and the pass. */
int cs_object_focus_last_timing(const cs_preproc *p, double *clear_ms, double *pass_ms);

/* ---- spots: local maxima of a difference of Gaussians, listed and counted per object ---------------------------------- */
/* Puncta in one channel (tests/spots_reference.py restates the rule, cellscreen/spots.py derives).  All integers.
 * Response.  A_t(i, j) = sum_k w_t[|k|] sum_l w_t[|l|] x(fold(i + k, height), fold(j + l, width)) for the two tables t = a (fine)
 *         and b (coarse) of cs_spot_params: cs_segment_smooth's separable 48-bit sum and its reflection (a radius may exceed a
 *         side).  R = (A_a - A_b + 2^23) >> 24, a floor shift of the signed difference: int32 in 1/256 counts, |R| < 2^24; a
 *         constant image has R = 0 everywhere.
 * Peaks.  The key of a pixel is (R, -raster index).  A pixel of image b is a spot iff R >= thresholds[b] and its key is strictly
 *         the greatest among the pixels with |dr| <= min_distance and |dc| <= min_distance, clipped to the image.  So no two spots
 *         lie within Chebyshev distance min_distance, and of a plateau the first pixel in raster order is the one that can be one.
 * Label.  labels[b][r][c], or 0 where exclude is non-zero there or labels is NULL.  Excluded pixels still take part in the
 *         response and in the window.
 * image:  [batch][height][width][channels] uint8 / uint16 (pixel_type), in_kind; params->channel is read.  height, width 1..4096,
 *         batch 1..65535 (above: CS_ERR_UNSUPPORTED); batch * height * width * 12 bytes of response scratch must stay under
 *         2^30 (else CS_ERR_UNSUPPORTED).
 * labels, exclude: NULL, or [batch][height][width] int32, in_kind; exclude needs labels.  With labels max_label >= 1 bounds them
 *         (batch * max_label above 2^22 or max_label above 2^20: CS_ERR_UNSUPPORTED); a negative label or one above max_label:
 *         CS_ERR_INVALID "negative or exceeds max_label", detected on the device, never an index or a key; the handle stays usable.
 * thresholds: [batch] int32 on the host, 1/256 counts, each >= 1 (else CS_ERR_INVALID).
 * counts: out, [batch][2] int64: the spots of the image, and those of them on label 0.
 * geom:   with labels out, [batch][max_label][3] int64: area, sum r, sum c -- cs_label_intensity's geom, bit for bit.
 * spots:  with labels out, [batch][max_label][CS_SPOT_RECORD] int64: n, sum R, sum R^2, max R (0 without a spot), sum r, sum c
 *         over the object's spots.  Without labels neither is written and both may be NULL.
 * response: NULL, or out, [batch][height][width] int32: R.  counts, geom, spots and response are out_kind.
 * n_spots: out, on the host: the length of the list, which stays on the handle until the next cs_spot_detect.  More than 2^22
 *         spots: CS_ERR_UNSUPPORTED, and no list.
 * cs_spot_fill copies out what the last successful cs_spot_detect on the handle left (none: CS_ERR_INVALID):
 * list:   out, [n_spots][CS_SPOT_FIELDS] int32: r, c, label, R, R(r-1, c), R(r+1, c), R(r, c-1), R(r, c+1), INT32_MIN for a
 *         neighbour outside the image; sorted by image, then raster order.  capacity: the spots the buffer holds, >= n_spots
 *         (else CS_ERR_INVALID); list may be NULL where capacity is 0.
 * offsets: out, [batch + 1] int64: the spots of image b are list[offsets[b] .. offsets[b + 1]).  Both out_kind.
 * No floating point and no float atomics: bit-identical run to run, whatever the launch geometry, and independent of the other
 * images of the batch.  Scratch from the buffers the handle's segmenter stages share; one host synchronisation per
 * cs_spot_detect.  Other bad arguments: CS_ERR_INVALID before any device work; without a gfx950 device (p == NULL):
 * CS_ERR_NO_DEVICE. */
#define CS_SPOT_RECORD 6
#define CS_SPOT_FIELDS 8
#define CS_SPOT_MAX_RADIUS 64
typedef struct cs_spot_params {
    int32_t radius_a;                 /* 0..64; 0: the identity, weights_a[0] = 65536 */
    int32_t radius_b;                 /* 1..64 */
    int32_t weights_a[CS_SPOT_MAX_RADIUS + 1];   /* both tables: non-negative, w[0] >= 1, 0 beyond the radius, */
    int32_t weights_b[CS_SPOT_MAX_RADIUS + 1];   /* w[0] + 2 * sum(w[1..radius]) == 65536; equal tables: CS_ERR_INVALID */
    int32_t min_distance;             /* 1..8: the window's half-width */
    int32_t channel;                  /* 0..channels - 1 */
    int32_t reserved;                 /* must be 0 */
} cs_spot_params;
int cs_spot_detect(cs_preproc *p, const void *image, int pixel_type, int32_t channels,
                   const int32_t *labels /* or NULL */, const int32_t *exclude /* or NULL */,
                   int32_t batch, int32_t height, int32_t width, int in_kind, int32_t max_label,
                   const cs_spot_params *params, const int32_t *thresholds, int64_t *counts,
                   int64_t *geom /* or NULL */, int64_t *spots /* or NULL */, int32_t *response /* or NULL */, int out_kind,
                   int64_t *n_spots);
int cs_spot_fill(cs_preproc *p, int32_t *list, int64_t capacity, int64_t *offsets, int out_kind);
/* Device time of the last cs_spot_detect: clearing + the response, the peaks with their counts, and the list with the records. */
int cs_spot_last_timing(const cs_preproc *p, double *response_ms, double *peaks_ms, double *records_ms);

/* ---- flat-field correction from a plate's own images ------------------------------------------------------------------ */
/* One multiplicative illumination function per channel, estimated from all fields of a plate and divided out of every field
 * (tests/illumination_reference.py restates the rule, cellscreen/illumination.py drives it) -- CellProfiler's
 * CorrectIlluminationCalculate / CorrectIlluminationApply.  All integers, no tolerance, bit-identical run to run.  The three
 * calls keep nothing between them: the caller owns the stack of meshes and the function.
 * The mesh is cs_segment_noise's: tile side T a power of two in 16..256, m = max(1, n / T) tiles along an axis of n pixels,
 * tile i = [i T, (i + 1) T), the last one runs to n.
 *
 * cs_illum_tile_stats: per image, channel and tile the value of rank (q_num (N - 1)) / q_den among the tile's N sorted pixels,
 *         0 <= q_num <= q_den <= 65536 (1 / 2: the lower median; 0: the minimum).
 * image:  [batch][height][width][channels] uint8 / uint16 (pixel_type), in_kind, channels 1..4 (more: CS_ERR_UNSUPPORTED).
 *         height, width 1..4096, batch 1..65535 (above: CS_ERR_UNSUPPORTED).
 * mesh:   out, [batch][channels][m_y][m_x] int32, out_kind.
 *
 * cs_illum_reduce: per channel and node, over the n stacked meshes (1 <= n <= 16384, above: CS_ERR_UNSUPPORTED), the value of
 *         rank (a_num (n - 1)) / a_den across the images, or with params->mean the rounded mean (2 sum + n) / (2 n); then
 *         F8 = 256 max(value - offset[c], floor); then, where asked for, the median of the 3 x 3 mesh neighbourhood (replicated
 *         edges) and a Gaussian over the mesh (cs_segment_smooth's table and reflection, one rounding (A + 2^31) >> 32 at the
 *         end, floored at 256 floor again).
 * stack:  [n][channels][m_y][m_x] int32, in_kind, every value 0..65535 (a host stack is checked and refused with
 *         CS_ERR_INVALID before any device work; a device stack: see the status words below).  m_y, m_x 1..256.
 * f8:     out, [channels][m_y][m_x] int32, out_kind: 256 <= F8 < 2^24.
 *
 * cs_illum_apply: y = clamp(pedestal[c] + floor((2 (v - offset[c]) G8[c] D + N) / (2 N)), 0, top) per pixel and channel: the
 *         quotient rounds half up and floors a negative numerator.  N = max(sum wy wx F8, 256 floor D) is F8 interpolated between
 *         the tile centres at the doubled coordinates C2_i = start_i + end_i - 1 and continued LINEARLY outside the outer ones
 *         (w1 = 2 p - C2_i is not clamped; cs_segment_noise continues constantly), D = Dy Dx, an axis with one node has D = 1.
 * image:  as above, `kind`; out: the same type, shape and `kind`, and may be image itself (in place).
 * f8:     [channels][m_y][m_x] int32 of (height, width, tile), mesh_kind; m_y, m_x are checked against them.  A host mesh with
 *         a value outside [256, 2^24) is CS_ERR_INVALID before any device work; a device mesh: see the status words below.
 * clipped: NULL, or out on the host, [batch][channels][2] int64: the pixels clamped at 0 and at top.
 * |w| < 5 T, so |sum| < 2^47 and the numerator stays below 2^62: everything is int64.
 * Status words.  A value of a device stack outside 0..65535, or of a device function outside [256, 2^24), is cut to that range
 * in the kernel (it is an operand, never an index) and raises a status word on the handle that only the host clears.  The call
 * itself answers CS_ERR_INVALID if it synchronises; if it does not, the handle's next cs_illum_* call that synchronises, or
 * cs_illum_last_timing, answers CS_ERR_INVALID in its place ("this call, or one before it that did not synchronise"), once.
 * The outputs of such a call are those of the cut values; the handle stays usable.
 * Host synchronisations: none when every buffer of a call is on the device and clipped is NULL (the result is complete in
 * stream order; cs_illum_last_timing waits for it), else one.  Uploads and tables on their way to the host go through the
 * buffers the handle's segmenter stages share.  Bad arguments (reserved words not 0 among them): CS_ERR_INVALID before any
 * device work; sides, batch or n above the caps: CS_ERR_UNSUPPORTED; without a gfx950 device (p == NULL): CS_ERR_NO_DEVICE. */
#define CS_ILLUM_MAX_RADIUS 64
#define CS_ILLUM_MAX_IMAGES 16384
typedef struct cs_illum_reduce_params {
    int32_t a_num, a_den;             /* 0 <= a_num <= a_den <= 65536, a_den >= 1; read without mean */
    int32_t mean;                     /* 0: the rank above, 1: the rounded mean */
    int32_t offset[4];                /* 0..65535 per channel: the camera's dark level in counts */
    int32_t floor;                    /* 1..4095 */
    int32_t mesh_median;              /* 0 or 1 */
    int32_t radius;                   /* 0: no Gaussian, else 1..64 */
    int32_t weights[CS_ILLUM_MAX_RADIUS + 1];    /* non-negative, w[0] >= 1, 0 beyond the radius, w[0] + 2 sum w[1..radius] == 65536 */
    int32_t reserved[2];              /* must be 0 */
} cs_illum_reduce_params;
typedef struct cs_illum_apply_params {
    int32_t tile;                     /* 16, 32, 64, 128 or 256 */
    int32_t floor;                    /* 1..4095 */
    int32_t g8[4];                    /* 1 <= G8 < 2^24 per channel */
    int32_t offset[4];                /* 0..65535 per channel */
    int32_t pedestal[4];              /* 0..65535 per channel */
    int32_t reserved[2];              /* must be 0 */
} cs_illum_apply_params;
int cs_illum_tile_stats(cs_preproc *p, const void *image, int pixel_type, int32_t channels,
                        int32_t batch, int32_t height, int32_t width, int in_kind, int32_t tile,
                        int32_t q_num, int32_t q_den, int32_t *mesh, int out_kind);
int cs_illum_reduce(cs_preproc *p, const int32_t *stack, int32_t n, int32_t channels, int32_t m_y, int32_t m_x, int in_kind,
                    const cs_illum_reduce_params *params, int32_t *f8, int out_kind);
int cs_illum_apply(cs_preproc *p, const void *image, int pixel_type, int32_t channels,
                   int32_t batch, int32_t height, int32_t width, int kind,
                   const int32_t *f8, int32_t m_y, int32_t m_x, int mesh_kind,
                   const cs_illum_apply_params *params, void *out, int64_t *clipped /* or NULL */);
/* Device time of the last cs_illum_tile_stats, cs_illum_reduce and cs_illum_apply on the handle.  Waits for a call that left
 * its result on the device, and reports the status words such a call raised (CS_ERR_INVALID; the times are written all the same). */
int cs_illum_last_timing(const cs_preproc *p, double *stats_ms, double *reduce_ms, double *apply_ms);

/* ---- detector fitting (create_anomaly_detector, CAE_improved_modeltrain.py:394-446) -------- */
/* The fit of what cs_screen's tail evaluates, for the training set's encoder features
 * (cs_encode output, [n][n_features] fp32, host or device).  Own handle, own stream.
 *   cs_fit_scaler       RobustScaler().fit (:408-409): center_ = per-feature median (float32), scale_ = 75th - 25th
 *                       percentile (float64, numpy's linear interpolation; spreads below 10 eps become 1).  Exact
 *                       (radix select of the order statistics + numpy's arithmetic on them).  NaNs and infinities:
 *                       CS_ERR_UNSUPPORTED.
 *   cs_fit_pca_moments  what PCA(...).fit (:412-414) needs from the data: mean_ (float32, numpy's row-after-row sum)
 *                       of the scaled features and the fp64 scatter matrix Xc^T Xc of the centred scaled features
 *                       ([F][F], host).  The principal axes are the leading eigenvectors of scatter / (n - 1); the
 *                       F x F eigenproblem is the host's (cellscreen/detector_fit.py uses LAPACK through numpy).
 *                       n_features must be a multiple of 128, at most 8192; wider features: cs_fit_pca_subspace.
 *   cs_fit_pca_subspace PCA(n_components).fit without anything F x F, for any n_features (1 .. 2^20): block subspace
 *                       iteration on the centred scaled features Xc with a Rayleigh-Ritz step (the class of
 *                       scikit-learn's randomized solver, which PCA(svd_solver='auto') picks for wide features).  A
 *                       seeded Gaussian block of L = min(128 (256 when n_components > 118), n_features, n - 1) columns;
 *                       per step Y = Xc Q, Z = Xc^T Y, Q = orth(Z) (CholeskyQR2, deficient columns replaced by fresh
 *                       random ones), all fp64 on the device; the host sees L x L matrices only.  Stops when no top-k
 *                       Ritz value of Q^T Xc^T Xc Q moves by more than 1e-5 relative, after at least scikit-learn's
 *                       'auto' iteration count (7, or 4 when n_components >= 0.1 min(n, F)) and at most 100 steps.
 *                       Outputs (host): mean [n_features] float32 (bit-identical to cs_fit_pca_moments'), components
 *                       [n_components][n_features] fp64 (descending variance, largest-magnitude entry of each row
 *                       positive), explained_variance [n_components], total_variance (sum of the column variances,
 *                       ddof 1), n_iter (power steps taken; may be NULL).  n_components: 1 .. min(128, n_features,
 *                       n - 1).  Same seed, same input: bit-identical results.
 *   cs_fit_project      scaler.transform + pca.transform of the training features with freshly fitted parameters
 *                       (the kernel cs_screen uses), out [n][n_components] fp32 on the host.
 *   cs_fit_ocsvm        OneClassSVM(kernel='rbf', nu).fit (:420-427): libsvm's SMO (second-order working-set selection,
 *                       Qfloat kernel rows, eps stopping rule) with every iteration on the device.  x: [n][n_components]
 *                       float64 host (what sklearn hands libsvm), gamma as resolved by sklearn ('scale':
 *                       1 / (n_components * x.var())), eps = tol (sklearn default 1e-3), max_iter < 0 = unbounded.
 *                       alpha: [n] dual variables (support vectors are the points with alpha > 0; dual_coef_ = alpha),
 *                       rho = -intercept_ = offset_.  status: 0 converged, 1 stopped at max_iter.  A solve that leaves rho
 *                       non-finite (nu = 1: every alpha at its bound) is CS_ERR_INVALID, as scikit-learn refuses it. */
typedef struct cs_fit cs_fit;
int cs_fit_create(int device_id, cs_fit **out);
void cs_fit_free(cs_fit *f);
int cs_fit_wait_stream(cs_fit *f, void *hip_stream);
int cs_fit_scaler(cs_fit *f, const float *features, int64_t n, int32_t n_features, int kind, float *center, double *scale);
int cs_fit_pca_moments(cs_fit *f, const float *features, int64_t n, int32_t n_features, int kind, const float *center,
                       const double *scale, float *mean, double *scatter);
int cs_fit_pca_subspace(cs_fit *f, const float *features, int64_t n, int32_t n_features, int kind, const float *center,
                        const double *scale, int32_t n_components, uint64_t seed, float *mean, double *components,
                        double *explained_variance, double *total_variance, int32_t *n_iter);
int cs_fit_project(cs_fit *f, const float *features, int64_t n, int32_t n_features, int kind, const float *center,
                   const double *scale, const float *components, const float *mean_proj, int32_t n_components, float *out);
int cs_fit_ocsvm(cs_fit *f, const double *x, int64_t n, int32_t n_components, double gamma, double nu, double eps,
                 int64_t max_iter, double *alpha, double *rho, double *obj, int64_t *n_iter, int32_t *status);
/* Device time (HIP events on the handle's stream) of the last cs_fit_* call, transfers of results included. */
int cs_fit_last_ms(const cs_fit *f, double *device_ms);

/* ---- measurement ---------------------------------------------------------------- */
/* When enabled, every kernel launch of this handle is bracketed by HIP events on the
 * handle's stream; totals are per kernel family.  Adds a stream sync per call. */
int cs_profile_enable(cs_model *m, int on);
int cs_profile_reset(cs_model *m);
int cs_profile_kernel_count(void);
const char *cs_profile_kernel_name(int kernel_id);
/* total_ms: summed device time; launches: number of launches; cells: cells processed;
 * flops: algorithmic FLOPs of those launches (2 x MACs of the reference graph). */
int cs_profile_get(cs_model *m, int kernel_id, double *total_ms, int64_t *launches,
                   int64_t *cells, double *flops);
/* Matrix-pipe instructions (v_mfma_f32_16x16x4_f32, 2,048 FLOP each) one cell costs in that kernel family with
 * the kernels this handle runs: the EXECUTED work a roofline fraction is priced with (Winograd / folded-upsample
 * kernels execute fewer multiply-adds than the layer's algorithmic count).  Equals SQ_INSTS_MFMA per cell. */
int cs_profile_mfma_per_cell(cs_model *m, int kernel_id, double *mfma);
/* The same for kernels that carry the fp32 contraction on the bf16 matrix pipe (three-way operand split, six
 * products: conv4 of the reference graph, the MFMA convs of other architectures): v_mfma_f32_16x16x32_bf16
 * instructions (16,384 FLOP each) per cell; such a kernel reports 0 from cs_profile_mfma_per_cell.
 * CS_NO_BF16X3=1 in the environment keeps every conv on the fp32 matrix instructions (A/B timing). */
int cs_profile_bf16_mfma_per_cell(cs_model *m, int kernel_id, double *mfma);

/* ---- training ---------------------------------------------------------------------- */
typedef struct cs_trainer cs_trainer;

/* Keras defaults of the reference: Adam(beta_1 0.9, beta_2 0.999, epsilon 1e-7)
 * (CAE_improved_modeltrain.py:224), BatchNormalization(momentum 0.99, epsilon 1e-3) (:192). */
typedef struct cs_train_cfg {
    float beta1, beta2, adam_eps;
    float bn_momentum, bn_eps;
} cs_train_cfg;

/* Number of trainable parameters (84,289) and of BatchNormalization moving statistics (512).
 * Flat layouts -- trainable: per conv l in order {kernel HWIO, bias, [gamma, beta]};
 * moving: per BN l in order {moving_mean, moving_variance}. */
int cs_train_param_count(int64_t *n_trainable, int64_t *n_moving);
/* The same two counts for the architecture of a handle (any instance of the layer grammar). */
int cs_train_param_count_of(const cs_trainer *t, int64_t *n_trainable, int64_t *n_moving);
/* init: starting weights + moving statistics (create_improved_autoencoder, :184-229).  The reference graph trains on
 * kernels tuned for it; any other instance of the layer grammar (see cs_model_from_arrays; additionally every filter
 * count but the last must divide 256) trains on run-time-shaped kernels (csrc/train_generic.hip) -- BASELINE.json
 * configs[4]'s 128x128 / 128-channel variant with the same forward_backward -> all-reduce -> apply split. */
int cs_train_create(const cs_cae_weights *init, const cs_train_cfg *cfg, int device_id, cs_trainer **out);
void cs_train_free(cs_trainer *t);
int cs_train_wait_stream(cs_trainer *t, void *hip_stream);
/* One fit() batch: forward (BN batch statistics, moving-average update), loss = mean((out-y)^2),
 * mae = mean|out-y|, backward, Adam update with learning rate lr.  x = network input (the
 * augmented image of datagen.flow(X_train, X_train), :287), y = target; [batch][H][W] fp32. */
int cs_train_step(cs_trainer *t, const float *x, const float *y, int64_t batch, int kind, float lr,
                  float *loss, float *mae);
/* The same batch with NO host synchronisation: copies, forward, backward, Adam and the operand re-pack are enqueued on the
 * handle's stream and the call returns.  The batch's loss / mae are added to running sums on the device -- Keras's epoch
 * metrics are the means over the epoch's batches (fit(), CAE_improved_modeltrain.py:286-293) -- and cs_train_read_metrics
 * fetches them: one host round trip per epoch instead of one per step.  x / y must stay valid until the step's input copies
 * have run; cs_train_inputs_consumed(t, stream) makes `stream` (the caller's, e.g. torch's current stream) wait for exactly
 * that point, and likewise for the device output of the last cs_train_augment.  Host batches fall back to a synchronous
 * step whose scalars are added on the host. */
int cs_train_step_async(cs_trainer *t, const float *x, const float *y, int64_t batch, int kind, float lr);
int cs_train_inputs_consumed(cs_trainer *t, void *hip_stream);
/* Mean loss / mae over the cs_train_step_async calls since the last reset, their number; reset != 0 clears the sums.
 * Synchronises the handle's stream. */
int cs_train_read_metrics(cs_trainer *t, double *loss_mean, double *mae_mean, int64_t *steps, int reset);
/* The two halves of cs_train_step, for data-parallel training: gradients are left in the
 * gradient buffer (all-reduce it between the two calls). */
int cs_train_forward_backward(cs_trainer *t, const float *x, const float *y, int64_t batch, int kind,
                              float *loss, float *mae);
int cs_train_apply(cs_trainer *t, float lr);
/* BatchNormalization over the WHOLE batch when the batch is split over `world` processes (the reference normalises over its
 * single batch of 32, CAE_improved_modeltrain.py:192-213 with batch_size=32 at :287).  cs_train_forward_backward then stops at
 * two points per BN layer -- after the layer's local {count, mean, M2} per channel (forward) and after its local
 * {sum dy, sum dy xhat} (backward) -- writes this rank's floats_per_rank values at device_buf + rank * floats_per_rank,
 * synchronises its stream and calls fn(ctx, floats_per_rank): the caller all-gathers in place (RCCL / torch.distributed; a
 * fake communicator in tests) and returns 0 once device_buf[0 .. world * floats_per_rank) is complete and visible to the
 * device.  The library merges the `world` triples in rank order (Chan's formula, double), so every rank gets identical
 * statistics, identical moving averages, and -- with the usual mean of the per-rank weight gradients -- the gradient of the
 * single-process step.  Every handle cs_train_create accepts can be synchronised: capacity_floats >= world * 3 * Cmax, Cmax being the
 * handle's largest BatchNormalization filter count (64 for the reference graph, up to 256); a smaller buffer is CS_ERR_INVALID and
 * the message names the floats needed.  fn == NULL switches synchronisation off.  Every rank must step the SAME number of cells: the
 * backward means divide by batch * world elements per pixel, so unequal per-rank batches are not supported.
 * A hook that returns non-zero fails the step with CS_ERR_INVALID.  The peers of that rank are then inside a collective that will
 * never complete: the caller must abort its process group (tear the communicator down), not merely retry the step. */
typedef int (*cs_allgather_fn)(void *ctx, int64_t floats_per_rank);
int cs_train_set_sync_bn(cs_trainer *t, cs_allgather_fn fn, void *ctx, float *device_buf, int64_t capacity_floats, int rank, int world);
/* The same exchange ORDERED ON THE STREAM, so that a synchronised step has one host wait (the loss read-back) as the single-GPU
 * step has.  fn must ENQUEUE an in-place all-gather of device_buf[0 .. world * floats_per_rank) so that it is ordered on hip_stream
 * (the handle's stream: run the collective on it, or on another stream tied to it by events in both directions) and return
 * without waiting for the device.  Work enqueued on hip_stream before the call wrote this rank's slot; work the library enqueues
 * after the call returns reads all slots.  With this hook the library calls no hipStreamSynchronize (or any other host wait)
 * between the input copies and the loss read-back of cs_train_forward_backward.  Buffer, rank / world, equal per-rank batches and
 * the failure contract are those of cs_train_set_sync_bn.  Registering either hook replaces the other; fn == NULL on either entry
 * point switches synchronisation off. */
typedef int (*cs_allgather_stream_fn)(void *ctx, int64_t floats_per_rank, void *hip_stream);
int cs_train_set_sync_bn_stream(cs_trainer *t, cs_allgather_stream_fn fn, void *ctx, float *device_buf, int64_t capacity_floats,
                                int rank, int world);
/* Use caller-owned device memory (n_trainable floats, e.g. a torch tensor) as the gradient
 * buffer; NULL restores the internal one. */
int cs_train_set_grad_buffer(cs_trainer *t, float *device_buffer);
/* Inference-mode loss / mae over n cells with the moving statistics (fit()'s validation pass). */
int cs_train_eval(cs_trainer *t, const float *x, const float *y, int64_t n, int kind, float *loss, float *mae);
/* Training augmentation: ImageDataGenerator(rotation_range=2, width/height_shift_range=0.02,
 * zoom_range=0.02, horizontal/vertical_flip, fill_mode='nearest') applied to the INPUT batch only
 * (CAE_improved_modeltrain.py:246-254, datagen.flow(X_train, X_train) at :287).
 * One transform per image, already reduced on the host to what
 * scipy.ndimage.affine_transform(order=1, mode='nearest') takes: input coordinate =
 * m . (row, col) + off, built in double exactly as Keras's apply_affine_transform does
 * (cellscreen/augment.py draws the parameters in Keras's order).  identity != 0 skips the
 * resampling (Keras does when no rotation/shift/zoom was drawn); flips come last. */
typedef struct cs_aug_affine {
    double m[4];      /* row-major 2x2 */
    double off[2];
    int32_t identity, flip_h, flip_v, reserved;
} cs_aug_affine;
/* x, out: [n][64][64] fp32, both `kind`; tf: host array of n transforms (copied before the call returns).  out may not
 * alias x.  A CS_MEM_DEVICE output is left on the handle's stream (the next cs_train_step* consumes it there); any other
 * reader orders itself with cs_train_inputs_consumed or a synchronising call.  CS_MEM_HOST returns when out is written. */
int cs_train_augment(cs_trainer *t, const float *x, int64_t n, const cs_aug_affine *tf, float *out, int kind);

/* The generator's settings (Keras names; CAE_improved_modeltrain.py:246-254 is {2, 0.02, 0.02, 0.98, 1.02, 1, 1, -0.5}).
 * Shift ranges below 1 are fractions of the image side, as in Keras; center: the transform's centre is size/2 + center. */
typedef struct cs_aug_config {
    double rotation_range;                        /* degrees: theta ~ U(-r, r) */
    double width_shift_range, height_shift_range;
    double zoom_lo, zoom_hi;                      /* zx, zy ~ U(lo, hi) each */
    int32_t horizontal_flip, vertical_flip;
    double center;
} cs_aug_config;
/* The n transforms of fit() step `step`: image b's seven draws (theta, tx = height shift, ty = width shift, zx, zy, flip_h,
 * flip_v -- Keras's get_random_transform order) are u(seed, step, b, j), j = 0..6, of a counter-based generator (three rounds
 * of splitmix64 over the key; cellscreen/augment.py has the same function), so a step's augmentation does not depend on how many
 * were drawn before it or on which rank draws it.  Host only, no device needed. */
int cs_train_draw_transforms(const cs_aug_config *aug, uint64_t seed, uint64_t step, int64_t n, int32_t height, int32_t width,
                             cs_aug_affine *out);
/* One fit() batch straight from a training set resident on the handle's device (CAE_improved_modeltrain.py:286-293:
 * datagen.flow(X_train, X_train, batch_size=32) -> one step of model.fit): gathers train[idx[b]], b < batch, draws the
 * batch's transforms (cs_train_draw_transforms; aug == NULL: none), resamples the INPUT only -- the target stays the original
 * crop -- and enqueues forward + backward + Adam like cs_train_step_async: no host synchronisation, no other call, no
 * intermediate tensor of the caller's.  idx: host array (copied before the call returns).  Metrics: cs_train_read_metrics. */
int cs_train_fit_step(cs_trainer *t, const float *train_device, int64_t n_train, const int32_t *idx, int64_t batch,
                      const cs_aug_config *aug, uint64_t seed, uint64_t step, float lr);

/* Copies to host (each pointer may be NULL): trainable parameters, moving statistics, last gradients. */
int cs_train_export(cs_trainer *t, float *params_host, float *moving_host, float *grads_host);
/* Stage tap for parity tests: copies one tensor of the last forward_backward to host.
 * which: 0 relu(conv) output, 1 BN(+pool) output, 2 dL/dz, 3 dL/d(BN output), 4 sigmoid output,
 * 5 the step's input, 6 the step's target (both batch x H x W floats, layer must be 0: what the last step -- for
 * cs_train_fit_step the gather and the resampling -- left in the handle's batch buffers).  Synchronises the handle's stream. */
int cs_train_tensor(cs_trainer *t, int which, int layer, int64_t batch, float *host);
/* Overwrites trainable parameters and/or moving statistics from host arrays (restore best weights). */
int cs_train_import(cs_trainer *t, const float *params_host, const float *moving_host);

#ifdef __cplusplus
}
#endif
#endif /* CELLSCREEN_H */
