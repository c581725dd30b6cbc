/* regSift3D -- match the SIFT3D features of two volumes and estimate the affine map between them, on the
 * MI355X.
 *
 * Same command line, outputs and messages as the reference program (cli/regSift3D.c:1-485):
 *     regSift3D [SIFT3D options] [--matches m.csv] [--transform t.csv] [--warped w.nii] [--nn_thresh v]
 *               [--err_thresh v] [--num_iter n] [--type affine] [--resample] source.nii reference.nii
 * and, beyond the reference, [--tps] [--tps_lambda v] [--tps_thresh v] [--tps_max_points n]: a thin-plate spline fitted to
 * the matches near the affine map (sift3d_amd_register_tps), written by --transform and used by --warped, and
 * [--metrics m.csv] [--metric_bins n]: the similarity of the images before and after (sift3d_amd_im_similarity), and
 * [--refine] [--refine_levels n] [--refine_iter n] [--refine_normalize]: the affine map improved on the voxel intensities
 * (sift3d_amd_refine_affine) before it is written, used by --warped and scored by --metrics, and
 * [--demons] [--demons_levels n] [--demons_iter n] [--demons_sigma s] [--demons_field f.nii]: a dense displacement field on top of
 * the affine map (sift3d_amd_register_demons), written by --demons_field and used by --warped, and
 * [--demons_inverse i.nii] [--demons_jacobian j.nii]: the inverse of that map as a field on the source grid
 * (sift3d_amd_invert_field) and the determinant of its Jacobian on the reference grid (sift3d_amd_field_jacobian),
 * linked against libsift3d_amd.so.  Detection, description, matching and the warp run as HIP kernels;
 * RANSAC is host C.  As in the reference, --err_thresh and --num_iter are parsed after the Ransac
 * parameters have been copied into the registration object, so they do not reach the estimator
 * (cli/regSift3D.c:176-178, 222-242).
 */
#include <getopt.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sift3d_amd.h"

static void usage(void)
{
    printf("Usage: regSift3D [source.nii] [reference.nii] \n"
           "\n"
           "Matches SIFT3D features. \n"
           "\n"
           "Supported input formats: \n"
           " .nii (nifti-1) \n"
           " .nii.gz (gzip-compressed nifti-1) \n"
           "\n"
           "Example: \n"
           " regSift3D --nn_thresh 0.8 --matches matches.csv src.nii ref.nii \n"
           "\n"
           "Output options: \n"
           " --matches [filename] - The feature matches. \n"
           "       Supported file formats: .csv, .csv.gz \n"
           " --transform [filename] - The transformation parameters. \n"
           "       Supported file formats: .csv, .csv.gz \n"
           " --warped [filename] -  The warped source image. \n"
           "       Supported file formats: .nii, .nii.gz \n"
           " --concat [filename] - Concatenated images, with source on the left \n"
           "       Supported file formats: .nii, .nii.gz \n"
           " --keys [filename] - Keypoints drawn in the concatenated image \n"
           "       Supported file formats: .nii, .nii.gz \n"
           " --lines [filename] - Lines drawn between matching keypoints \n"
           "       Supported file formats: .nii, .nii.gz \n"
           "At least one output option must be specified. \n"
           "\n"
           "Thin-plate-spline options: \n"
           " --tps - After the affine fit, fit a thin-plate spline to the \n"
           "       matches that agree with it. --transform then writes the \n"
           "       spline (one row [x y z wx wy wz] per control point, then \n"
           "       four rows [0 0 0 ax ay az]: the constant and the x, y, z \n"
           "       coefficients) and --warped warps with it. \n"
           " --tps_lambda [value] - Smoothing weight, in the interval \n"
           "       [0, inf). 0 interpolates the matches. (default: %.0f) \n"
           " --tps_thresh [value] - Matches within this distance of the \n"
           "       affine fit, in real-world units, become control points. \n"
           "       (default: 4 x err_thresh) \n"
           " --tps_max_points [value] - Largest number of control points. \n"
           "       (default: %d) \n"
           "\n"
           "Similarity options: \n"
           " --metrics [filename] - How well the images agree, one row per \n"
           "       stage: before registration, under the affine fit and, \n"
           "       with --tps or --refine, under the spline or the refined \n"
           "       map. Columns: n (voxels of the overlap), n_total, mse, \n"
           "       mae, ncc, mi, nmi. \n"
           "       Supported file formats: .csv, .csv.gz \n"
           " --metric_bins [value] - Bins per axis of the joint histogram \n"
           "       behind mi and nmi, in the interval [2, %d]. (default: %d) \n"
           "\n"
           "Refinement options: \n"
           " --refine - After the affine fit, improve it on the voxel \n"
           "       intensities (Levenberg-Marquardt on the squared \n"
           "       difference over the overlap, coarse to fine). \n"
           "       --transform and --warped then use the refined map and \n"
           "       --metrics gets a row for it. \n"
           " --refine_levels [value] - Pyramid levels, at least 1. \n"
           "       (default: %d) \n"
           " --refine_iter [value] - Largest number of accepted steps per \n"
           "       level, at least 1. (default: %d) \n"
           " --refine_normalize - Compare z-scored intensities: for images \n"
           "       that differ by a gain and an offset. \n"
           "\n"
           "Deformable options: \n"
           " --demons - After the affine fit (and --refine, if given), \n"
           "       register what is left on the voxel intensities: a dense \n"
           "       displacement field by Thirion's demons, coarse to fine. \n"
           "       --warped then warps through the affine map plus the \n"
           "       field. --transform still writes the affine map. \n"
           " --demons_levels [value] - Pyramid levels, at least 1. \n"
           "       (default: %d) \n"
           " --demons_iter [value] - Largest number of passes per level, \n"
           "       at least 1. (default: %d) \n"
           " --demons_sigma [value] - Smoothing of the field per pass, in \n"
           "       voxels of the level, in the interval [0.5, 8]. \n"
           "       (default: 1.5) \n"
           " --demons_field [filename] - The displacement field on the \n"
           "       reference grid, in source voxels: a 4-D image with the \n"
           "       x, y and z components as channels. \n"
           "       Supported file formats: .nii, .nii.gz \n"
           " --demons_inverse [filename] - The inverse of the map, as a \n"
           "       displacement field on the source grid, in reference \n"
           "       voxels, on top of the inverse affine map: a 4-D image \n"
           "       like --demons_field. \n"
           "       Supported file formats: .nii, .nii.gz \n"
           " --demons_jacobian [filename] - The determinant of the map's \n"
           "       Jacobian on the reference grid, in voxel coordinates. \n"
           "       Values <= 0 mark voxels where the map folds. \n"
           "       Supported file formats: .nii, .nii.gz \n"
           "\n"
           "Other options: \n"
           " --nn_thresh [value] - Matching threshold on the nearest neighbor \n"
           "       ratio, in the interval (0, 1]. (default: %.2f) \n"
           " --err_thresh [value] - RANSAC inlier threshold, in the interval \n"
           "       (0, inf). This is a threshold on the squared Euclidean \n"
           "       distance in real-world units. (default: %.1f) \n"
           " --num_iter [value] - Number of RANSAC iterations. (default: %d) \n"
           " --type [value] - Type of transformation to be applied. \n"
           "       Supported arguments: \"affine\" (default: affine) \n"
           " --resample - Internally resample the images to have the same \n"
           "	physical resolution. This is slow. Use it when the images \n"
           "	have very different resolutions, for example registering 5mm \n"
           "	to 1mm slices. \n"
           "\n",
           SIFT3D_AMD_TPS_LAMBDA_DEFAULT, SIFT3D_AMD_TPS_MAX_POINTS_DEFAULT, SIFT3D_AMD_SIMILARITY_BINS_MAX,
           SIFT3D_AMD_SIMILARITY_BINS_DEFAULT, SIFT3D_AMD_REFINE_LEVELS_DEFAULT, SIFT3D_AMD_REFINE_ITER_DEFAULT,
           SIFT3D_AMD_DEMONS_LEVELS_DEFAULT, SIFT3D_AMD_DEMONS_ITER_DEFAULT, SIFT3D_nn_thresh_default,
           SIFT3D_err_thresh_default, SIFT3D_num_iter_default);
    print_opts_SIFT3D();
}

static void complain(const char *msg)
{
    fprintf(stderr, "regSift3D: %s \nUse \"regSift3D --help\" for more information. \n", msg);
}

static void complain_bug(const char *msg)
{
    complain(msg);
    print_bug_msg();
}

static void complain_path(const char *what, const char *path)
{
    char msg[1024];
    snprintf(msg, sizeof(msg), "%s \"%s\"", what, path);
    complain(msg);
}

int main(int argc, char *argv[])
{
    enum { MATCHES = 'a', TRANSFORM, WARPED, CONCAT, KEYS, LINES, NN_THRESH, ERR_THRESH, NUM_ITER, TYPE, RESAMPLE, TPS_FIT, TPS_LAMBDA,
           TPS_THRESH, TPS_MAX_POINTS, METRICS, METRIC_BINS, REFINE, REFINE_LEVELS, REFINE_ITER, REFINE_NORMALIZE,
           DEMONS, DEMONS_LEVELS, DEMONS_ITER, DEMONS_SIGMA, DEMONS_FIELD, DEMONS_INVERSE, DEMONS_JACOBIAN };
    static const struct option longopts[] = {{"matches", required_argument, NULL, MATCHES},
                                             {"transform", required_argument, NULL, TRANSFORM},
                                             {"warped", required_argument, NULL, WARPED},
                                             {"concat", required_argument, NULL, CONCAT},
                                             {"keys", required_argument, NULL, KEYS},
                                             {"lines", required_argument, NULL, LINES},
                                             {"nn_thresh", required_argument, NULL, NN_THRESH},
                                             {"err_thresh", required_argument, NULL, ERR_THRESH},
                                             {"num_iter", required_argument, NULL, NUM_ITER},
                                             {"type", required_argument, NULL, TYPE},
                                             {"resample", no_argument, NULL, RESAMPLE},
                                             {"tps", no_argument, NULL, TPS_FIT},
                                             {"tps_lambda", required_argument, NULL, TPS_LAMBDA},
                                             {"tps_thresh", required_argument, NULL, TPS_THRESH},
                                             {"tps_max_points", required_argument, NULL, TPS_MAX_POINTS},
                                             {"metrics", required_argument, NULL, METRICS},
                                             {"metric_bins", required_argument, NULL, METRIC_BINS},
                                             {"refine", no_argument, NULL, REFINE},
                                             {"refine_levels", required_argument, NULL, REFINE_LEVELS},
                                             {"refine_iter", required_argument, NULL, REFINE_ITER},
                                             {"refine_normalize", no_argument, NULL, REFINE_NORMALIZE},
                                             {"demons", no_argument, NULL, DEMONS},
                                             {"demons_levels", required_argument, NULL, DEMONS_LEVELS},
                                             {"demons_iter", required_argument, NULL, DEMONS_ITER},
                                             {"demons_sigma", required_argument, NULL, DEMONS_SIGMA},
                                             {"demons_field", required_argument, NULL, DEMONS_FIELD},
                                             {"demons_inverse", required_argument, NULL, DEMONS_INVERSE},
                                             {"demons_jacobian", required_argument, NULL, DEMONS_JACOBIAN},
                                             {0, 0, 0, 0}};
    Reg_SIFT3D reg;
    SIFT3D sift3d;
    Ransac ran;
    Image src, ref;
    Mat_rm match_src, match_ref;
    Affine tform;
    Tps tps;
    sift3d_amd_tps_opts tps_opts = {-1.0, 0.0, 0};     /* the library's defaults */
    const char *match_path = NULL, *tform_path = NULL, *warped_path = NULL, *concat_path = NULL, *keys_path = NULL,
               *lines_path = NULL, *metrics_path = NULL, *field_path = NULL, *inverse_path = NULL, *jacobian_path = NULL;
    sift3d_amd_similarity_opts sim_opts = {0, LINEAR, {0.0, 0.0}, {0.0, 0.0}};   /* the library's defaults */
    sift3d_amd_refine_opts refine_opts = {0, 0, 0.0, 0.0, 0};                    /* the library's defaults */
    sift3d_amd_demons_opts demons_opts = {0, 0, 0.0, 0.0, 0.0, 0.0, 0};          /* the library's defaults */
    int have_match = 0, have_tform = 0, resample = 0, use_tps = 0, refine = 0, demons = 0;

    switch (parse_gnu(argc, argv)) {
    case SIFT3D_HELP: usage(); return 0;
    case SIFT3D_VERSION: return 0;
    case SIFT3D_FALSE: break;
    default: complain_bug("Unexpected return from parse_gnu."); return 1;
    }
    init_im(&src);
    init_im(&ref);
    init_Reg_SIFT3D(&reg);
    init_Ransac(&ran);
    if (init_SIFT3D(&sift3d) || init_Mat_rm(&match_src, 0, 0, SIFT3D_DOUBLE, SIFT3D_FALSE) ||
        init_Mat_rm(&match_ref, 0, 0, SIFT3D_DOUBLE, SIFT3D_FALSE)) {
        complain_bug("Failed basic initialization.");
        return 1;
    }
    if ((argc = parse_args_SIFT3D(&sift3d, argc, argv, SIFT3D_FALSE)) < 0) return 1;
    if (set_SIFT3D_Reg_SIFT3D(&reg, &sift3d) || set_Ransac_Reg_SIFT3D(&reg, &ran)) {
        complain_bug("Failed to save the SIFT3D or Ransac parameters.");
        return 1;
    }
    opterr = 1;
    for (int c; (c = getopt_long(argc, argv, "", longopts, NULL)) != -1;) {
        switch (c) {
        case MATCHES: match_path = optarg; have_match = 1; break;
        case TRANSFORM: tform_path = optarg; have_tform = 1; break;
        case WARPED: warped_path = optarg; have_tform = 1; break;
        case CONCAT: concat_path = optarg; have_match = 1; break;
        case KEYS: keys_path = optarg; have_match = 1; break;
        case LINES: lines_path = optarg; have_match = 1; break;
        case NN_THRESH:
            if (set_nn_thresh_Reg_SIFT3D(&reg, atof(optarg))) { complain("Invalid value for nn_thresh."); return 1; }
            break;
        case ERR_THRESH:
            if (set_err_thresh_Ransac(&ran, atof(optarg))) { complain("Invalid value for err_thresh."); return 1; }
            break;
        case NUM_ITER:
            if (set_num_iter_Ransac(&ran, atoi(optarg))) { complain("Invalid value for num_iter."); return 1; }
            break;
        case TYPE:
            if (strcmp(optarg, "affine")) {
                char msg[1024];
                snprintf(msg, sizeof(msg), "Unrecognized transformation type: %s", optarg);
                complain(msg);
                return 1;
            }
            break;
        case RESAMPLE: resample = 1; break;
        case TPS_FIT: use_tps = 1; break;
        case TPS_LAMBDA:
            tps_opts.lambda = atof(optarg);
            if (!(tps_opts.lambda >= 0.0)) { complain("Invalid value for tps_lambda."); return 1; }
            break;
        case TPS_THRESH:
            tps_opts.ctrl_thresh = atof(optarg);
            if (!(tps_opts.ctrl_thresh > 0.0)) { complain("Invalid value for tps_thresh."); return 1; }
            break;
        case TPS_MAX_POINTS:
            tps_opts.max_points = atoi(optarg);
            if (tps_opts.max_points < 4) { complain("Invalid value for tps_max_points."); return 1; }
            break;
        case METRICS: metrics_path = optarg; have_tform = 1; break;
        case METRIC_BINS:
            sim_opts.bins = atoi(optarg);
            if (sim_opts.bins < 2 || sim_opts.bins > SIFT3D_AMD_SIMILARITY_BINS_MAX) { complain("Invalid value for metric_bins."); return 1; }
            break;
        case REFINE: refine = 1; break;
        case REFINE_LEVELS:
            refine_opts.levels = atoi(optarg);
            if (refine_opts.levels < 1) { complain("Invalid value for refine_levels."); return 1; }
            break;
        case REFINE_ITER:
            refine_opts.max_iter = atoi(optarg);
            if (refine_opts.max_iter < 1) { complain("Invalid value for refine_iter."); return 1; }
            break;
        case REFINE_NORMALIZE: refine_opts.normalize = 1; break;
        case DEMONS: demons = 1; break;
        case DEMONS_LEVELS:
            demons_opts.levels = atoi(optarg);
            if (demons_opts.levels < 1) { complain("Invalid value for demons_levels."); return 1; }
            break;
        case DEMONS_ITER:
            demons_opts.max_iter = atoi(optarg);
            if (demons_opts.max_iter < 1) { complain("Invalid value for demons_iter."); return 1; }
            break;
        case DEMONS_SIGMA:
            demons_opts.sigma = atof(optarg);
            if (!(demons_opts.sigma >= 0.5 && demons_opts.sigma <= 8.0)) { complain("Invalid value for demons_sigma."); return 1; }
            break;
        case DEMONS_FIELD: field_path = optarg; have_tform = 1; break;
        case DEMONS_INVERSE: inverse_path = optarg; have_tform = 1; break;
        case DEMONS_JACOBIAN: jacobian_path = optarg; have_tform = 1; break;
        default: return 1;
        }
    }
    if (!have_match && !have_tform) { complain("No outputs were specified."); return 1; }
    if (argc - optind < 2) { complain("Not enough arguments."); return 1; }
    if (argc - optind > 2) { complain("Too many arguments."); return 1; }
    const char *src_path = argv[optind], *ref_path = argv[optind + 1];
    if (use_tps && resample) { complain("--tps cannot be combined with --resample."); return 1; }
    if (metrics_path != NULL && resample) { complain("--metrics cannot be combined with --resample."); return 1; }
    if (refine && resample) { complain("--refine cannot be combined with --resample."); return 1; }
    if (refine && use_tps) { complain("--refine cannot be combined with --tps."); return 1; }
    if (demons && use_tps) { complain("--demons cannot be combined with --tps."); return 1; }
    if (demons && resample) { complain("--demons cannot be combined with --resample."); return 1; }
    if (field_path != NULL && !demons) { complain("--demons_field needs --demons."); return 1; }
    if (inverse_path != NULL && !demons) { complain("--demons_inverse needs --demons."); return 1; }
    if (jacobian_path != NULL && !demons) { complain("--demons_jacobian needs --demons."); return 1; }
    /* the field only shows in --warped and the --demons_.. outputs */
    demons = demons && (warped_path != NULL || field_path != NULL || inverse_path != NULL || jacobian_path != NULL);
    refine = refine && have_tform;                     /* the refined map only shows in --transform, --warped and --metrics */
    use_tps = use_tps && have_tform;                   /* the spline only shows in --transform, --warped and --metrics */
    if (init_tform(&tform, AFFINE) || init_Tps(&tps, IM_NDIMS, IM_NDIMS + 1)) return 1;
    if (im_read(src_path, &src)) { complain_path("Failed to read the source image", src_path); return 1; }
    if (im_read(ref_path, &ref)) { complain_path("Failed to read the reference image", ref_path); return 1; }
    void *const tform_arg = have_tform ? (void *)&tform : NULL;
    if (resample) {
        if (register_SIFT3D_resample(&reg, &src, &ref, LINEAR, tform_arg)) {
            complain("Failed to register the images with resampling. \n");
            return 1;
        }
    } else {
        if (set_src_Reg_SIFT3D(&reg, &src)) { complain("Failed to set the source image."); return 1; }
        if (set_ref_Reg_SIFT3D(&reg, &ref)) { complain("Failed to set the reference image."); return 1; }
        if (use_tps) {
            if (sift3d_amd_register_tps(&reg, &tps_opts, &tform, &tps)) {
                fprintf(stderr, "%s\n", sift3d_amd_last_error());
                complain("Failed to register the images with a thin-plate spline.");
                return 1;
            }
        } else if (register_SIFT3D(&reg, tform_arg)) { complain("Failed to register the images."); return 1; }
    }
    if (get_matches_Reg_SIFT3D(&reg, &match_src, &match_ref)) {
        complain_bug("Failed to convert matches to coordinates.");
        return 1;
    }
    if (match_path != NULL) {
        Mat_rm matches;
        init_Mat_rm(&matches, 0, 0, SIFT3D_DOUBLE, SIFT3D_FALSE);
        if (concat_Mat_rm(&match_src, &match_ref, &matches, 1)) { complain_bug("Failed to concatenate the matches."); return 1; }
        if (write_Mat_rm(match_path, &matches)) { complain_path("Failed to write the matches", match_path); return 1; }
        cleanup_Mat_rm(&matches);
    }
    Affine refined;                                    /* tform stays the keypoint fit: --metrics scores both */
    if (init_tform(&refined, AFFINE)) return 1;
    if (refine) {
        sift3d_amd_refine_info rinfo;
        if (copy_tform(&tform, &refined) || sift3d_amd_refine_affine(&src, &ref, &refine_opts, &refined, &rinfo)) {
            fprintf(stderr, "%s\n", sift3d_amd_last_error());
            complain("Failed to refine the affine transformation.");
            return 1;
        }
    }
    const void *const tform_out = refine ? (const void *)&refined : use_tps ? (const void *)&tps : (const void *)&tform;
    if (tform_path != NULL && write_tform(tform_path, tform_out)) {
        complain_path("Failed to write the transformation parameters", tform_path);
        return 1;
    }
    Image field;                                       /* on top of tform_out; --transform and --metrics keep to the affine map */
    init_im(&field);
    if (demons) {
        sift3d_amd_demons_info dinfo;
        if (sift3d_amd_register_demons(&src, &ref, tform_out, &demons_opts, &field, &dinfo)) {
            fprintf(stderr, "%s\n", sift3d_amd_last_error());
            complain("Failed to register the images with a displacement field.");
            return 1;
        }
        if (field_path != NULL && im_write(field_path, &field)) { complain_path("Failed to write the displacement field", field_path); return 1; }
        if (inverse_path != NULL || jacobian_path != NULL) {   /* both are computed, for the line below: they cost a pass each */
            const double src_units[3] = {src.ux, src.uy, src.uz};
            sift3d_amd_field_inverse_info iinfo;
            sift3d_amd_field_jacobian_info jinfo;
            Affine inv_tform;
            Image inv_field, det;
            init_im(&inv_field);
            init_im(&det);
            if (init_tform(&inv_tform, AFFINE)) return 1;
            if (sift3d_amd_invert_field(tform_out, &field, src.nx, src.ny, src.nz, src_units, NULL, &inv_tform, &inv_field, &iinfo) ||
                sift3d_amd_field_jacobian(tform_out, &field, jacobian_path != NULL ? &det : NULL, &jinfo)) {
                fprintf(stderr, "%s\n", sift3d_amd_last_error());
                complain("Failed to invert the displacement field or to map its Jacobian.");
                return 1;
            }
            printf("Deformation: %lld folded voxels of %lld, minimum determinant %g; inverse: %lld converged, %lld not converged "
                   "of %lld. \n", jinfo.n_folded, jinfo.n, jinfo.min_det, iinfo.n_converged + iinfo.n_outside, iinfo.n_not_converged,
                   iinfo.n);
            if (inverse_path != NULL && im_write(inverse_path, &inv_field)) { complain_path("Failed to write the inverse field", inverse_path); return 1; }
            if (jacobian_path != NULL && im_write(jacobian_path, &det)) { complain_path("Failed to write the determinant map", jacobian_path); return 1; }
            im_free(&inv_field); im_free(&det);
            cleanup_tform(&inv_tform);
        }
    }
    if (metrics_path != NULL) {                        /* one row per stage, on the images as read */
        const void *const stages[3] = {NULL, &tform, refine ? (const void *)&refined : (const void *)&tps};
        const int nstages = use_tps || refine ? 3 : 2;
        Mat_rm metrics;
        if (init_Mat_rm(&metrics, nstages, 7, SIFT3D_DOUBLE, SIFT3D_TRUE)) { complain_bug("Failed to allocate the metrics."); return 1; }
        for (int i = 0; i < nstages; i++) {
            sift3d_amd_similarity sim;
            if (sift3d_amd_im_similarity(stages[i], &src, &ref, &sim_opts, &sim, NULL)) {
                complain("Failed to compute the similarity of the images.");
                return 1;
            }
            double *const row = metrics.u.data_double + (size_t)i * 7;
            row[0] = (double)sim.n; row[1] = (double)sim.n_total; row[2] = sim.mse; row[3] = sim.mae; row[4] = sim.ncc;
            row[5] = sim.mi; row[6] = sim.nmi;
        }
        if (write_Mat_rm(metrics_path, &metrics)) { complain_path("Failed to write the metrics", metrics_path); return 1; }
        cleanup_Mat_rm(&metrics);
    }
    if (warped_path != NULL) {
        Image warped;
        init_im(&warped);
        if (im_copy_dims(&ref, &warped)) { complain_bug("Failed to resize the warped image."); return 1; }
        if (demons ? sift3d_amd_im_warp_field(tform_out, &field, &src, LINEAR, &warped)
                   : im_inv_transform(tform_out, &src, LINEAR, SIFT3D_FALSE, &warped)) {
            complain_bug("Failed to warp the source image.");
            return 1;
        }
        if (im_write(warped_path, &warped)) { complain_path("Failed to write the warped image", warped_path); return 1; }
        im_free(&warped);
    }
    if (concat_path != NULL || keys_path != NULL || lines_path != NULL) {
        Image concat, keys, lines;
        Mat_rm keys_src, keys_ref;
        init_im(&concat);
        init_im(&keys);
        init_im(&lines);
        if (init_Mat_rm(&keys_src, 0, 0, SIFT3D_DOUBLE, SIFT3D_FALSE) || init_Mat_rm(&keys_ref, 0, 0, SIFT3D_DOUBLE, SIFT3D_FALSE)) {
            complain_bug("Failed to initialize keypoint matrices.");
            return 1;
        }
        if (SIFT3D_Descriptor_coords_to_Mat_rm(&reg.desc_src, &keys_src) ||
            SIFT3D_Descriptor_coords_to_Mat_rm(&reg.desc_ref, &keys_ref)) {
            complain_bug("Failed to convert the keypoints to matrices.");
            return 1;
        }
        if (draw_matches(&src, &ref, &keys_src, &keys_ref, &match_src, &match_ref, concat_path ? &concat : NULL,
                         keys_path ? &keys : NULL, lines_path ? &lines : NULL)) {
            complain_bug("Failed to draw the matches.");
            return 1;
        }
        if (concat_path != NULL && im_write(concat_path, &concat)) { complain_path("Failed to write the concatenated image", concat_path); return 1; }
        if (keys_path != NULL && im_write(keys_path, &keys)) { complain_path("Failed to write the keypoint image", keys_path); return 1; }
        if (lines_path != NULL && im_write(lines_path, &lines)) { complain_path("Failed to write the line image", lines_path); return 1; }
        im_free(&concat); im_free(&keys); im_free(&lines);
        cleanup_Mat_rm(&keys_src); cleanup_Mat_rm(&keys_ref);
    }
    cleanup_tform(&tform);
    cleanup_tform(&tps);
    cleanup_tform(&refined);
    im_free(&field);
    cleanup_Mat_rm(&match_src);
    cleanup_Mat_rm(&match_ref);
    cleanup_Reg_SIFT3D(&reg);
    cleanup_SIFT3D(&sift3d);
    im_free(&src);
    im_free(&ref);
    return 0;
}
