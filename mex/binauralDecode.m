function binauralOut = binauralDecode(in, inFs, decodingFilterLeft, decodingFilterRight, decodingFilterFs, compensateDelay, signal, signalFs, horRotAngleRad, shDefinition, rotationDomain, pitchRad, rollRad)
% dependencies/binauralDecode.m:1-64 on the GPU: real or complex SH (or CH) signals and filters, the yaw rotation of the input
% (a scalar, or one angle per input sample) and the convolution with a dry source signal.  The resampling (:12-23) uses the
% Signal Processing Toolbox's resample where it is installed, and emaglsResample (the library's restatement of it) otherwise.
% shDefinition ('real', the basis rotateHOA_N3D assumes, or 'complex') and rotationDomain ('sh' or 'ch') go beyond the reference.
% pitchRad and rollRad (optional, SH only): the other two angles of rotateHOA_N3D, each a scalar or one angle per input sample
% (see rotateSH).
if nargin > 6 && ~isempty(signal) && signalFs ~= inFs
    disp('binauralDecode: resampling signal');
    signal = resampleAny(signal, inFs, signalFs);
end
if decodingFilterFs ~= inFs
    disp('binauralDecode: resampling decoding filter');
    decodingFilterLeft = resampleAny(decodingFilterLeft, inFs, decodingFilterFs);
    decodingFilterRight = resampleAny(decodingFilterRight, inFs, decodingFilterFs);
end
comp = nargin > 5 && compensateDelay;
if isreal(decodingFilterLeft) ~= isreal(decodingFilterRight)      % both real or both complex at the boundary
    decodingFilterLeft = complex(decodingFilterLeft); decodingFilterRight = complex(decodingFilterRight);
end
if nargin < 7; signal = []; end
if nargin < 9; horRotAngleRad = []; end
if nargin < 10; shDefinition = 'real'; end
if nargin < 11; rotationDomain = 'sh'; end
% the library rotates (:27-31), decodes, convolves with signal(:,1) (:44-48), cuts the delay of the decoding filters (:53-57) and
% sums the discarded imaginary part over the samples it returns (:59-62)
if nargin < 12; pitchRad = []; end
if nargin < 13; rollRad = []; end
[binauralOut, imagSum] = emagls_mex('decode', double(in), double(decodingFilterLeft), double(decodingFilterRight), logical(comp), ...
                                    double(horRotAngleRad), double(signal), shDefinition, rotationDomain, double(pitchRad), double(rollRad));
% :59-63, the reference's text; it fires when the accumulated result is complex, i.e. has a non-zero imaginary part
if any(imagSum ~= 0)
    warning('discarding imaginary part with sum of [%.2g, %.2g] in rendering result.', imagSum(1), imagSum(2));
end
end

function y = resampleAny(x, p, q)
% the toolbox's resample when it exists (no change for its users), the GPU restatement otherwise
if exist('resample') == 2
    y = resample(x, p, q);
else
    y = emaglsResample(x, p, q);
end
end
